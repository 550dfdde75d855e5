// capi.hip -- the extern "C" boundary of libvo_hip.so (see include/vo_hip.h).
// Host-side plumbing only: argument checks, device buffers, uploads, launches.
// There is no CPU implementation of any operator behind these entry points.
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <map>
#include <mutex>
#include <set>
#include <tuple>
#include <vector>

#include "capi_internal.h"
#include "../../include/vo/epipolar.hpp"   // host linear algebra of vo_estimate_transform

using namespace vo;

namespace {

thread_local char g_err[512] = "";

int fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}
void set_error_v(const char* fmt, va_list ap) { vsnprintf(g_err, sizeof(g_err), fmt, ap); }

}  // namespace

int vo_fail(int code, const char* fmt, ...) {        // for the other translation units (vo_internal.h)
  va_list ap;
  va_start(ap, fmt);
  set_error_v(fmt, ap);
  va_end(ap);
  return code;
}

struct vo_event {
  int device = 0;
  hipEvent_t ev = nullptr;
};

// Contexts that exist.  Solvers, graphs and kd-trees keep a pointer to the context they were made on; the header asks for
// them to be destroyed first, but destruction order is easy to get wrong in a host program (statics, members, scripting
// languages), so a handle that outlives its context must fail cleanly when used and must still be destroyable.
static std::mutex g_ctx_mu;
static std::set<const vo_ctx*> g_ctx_live;
static unsigned long long g_ctx_next_id = 1;
bool ctx_alive(const vo_ctx* c) {
  std::lock_guard<std::mutex> lk(g_ctx_mu);
  return c && g_ctx_live.count(c) != 0;
}
// the context a handle was made on: still there, and still THAT context (not a new one at the recycled address)
bool ctx_alive(const vo_ctx* c, unsigned long long id) {
  std::lock_guard<std::mutex> lk(g_ctx_mu);
  return c && g_ctx_live.count(c) != 0 && c->id == id;
}

struct vo_graph {
  vo_ctx* ctx = nullptr;
  unsigned long long ctx_id = 0;
  hipGraphExec_t exec = nullptr;
};

// a handle whose tail launches run real rounds goes back to a launch per round and tries the form again with one solve in
// PICP_TAIL_PROBE_EVERY, then in twice as many after every probe that ran real rounds again, up to PICP_TAIL_PROBE_MAX
constexpr int PICP_TAIL_PROBE_EVERY = 1024, PICP_TAIL_PROBE_MAX = 65536;
struct vo_picp {
  vo_ctx* ctx = nullptr;
  unsigned long long ctx_id = 0;
  PicpParams hp;               // host mirror of the device parameters
  PicpParams* d_params = nullptr;
  PicpState* d_state = nullptr;
  bool params_dirty = true;
  DevBuf world_own{true}, meas_own{true}, pairs_own{true};   // keeps_state: the host forms' points and pairs, from the call that set them to the solves that read them
  DevBuf packed;               // (re-packed whenever it is ensured: packed_valid)
  DevBuf partials{true};       // keeps_state: rows >= grid are never written and must read as zero (zeroed_for_grid)
  const float* d_world = nullptr;
  const float* d_meas = nullptr;
  int n_world = 0, n_meas = 0;
  bool have_points = false;
  // host copy of the correspondences already uploaded and packed: a call whose pairs compare equal to it
  // (whole array, memcmp) skips the upload; anything else -- including an in-place edit -- is re-uploaded
  std::vector<int32_t> shadow;
  bool shadow_valid = false;
  bool packed_valid = false;
  int exact = 0;              // reference-order arithmetic (picp_exact_kernel)
  int set_n = -1;             // pair count handed over by vo_picp_set_correspondences
  int grid = 1;
  const float* pending_T0 = nullptr;   // device 4x4 to load as the pose by the next pack launch
  // A solve in the fast mode gathers in its first round (launch_picp_rounds): picp_prepare leaves what the pack launch would
  // have got here (on = 1), and the picp_enqueue that follows it in the same call consumes it.
  PicpGather gather;
  int zeroed_for_grid = -1;   // grid the (zero-padded) partial buffers were last cleared for
  // Rounds enqueued since the state (pose[0], T16, H, b, statistics) was last complete: vo_picp_one_round enqueues ONE
  // launch per call and leaves the finishing launch to whoever needs the state next (a getter, a setter, a multi-round
  // solve): picp_flush.  0 = the state is complete.
  int chain_len = 0;
  // Rounds enqueued BEYOND chain_len: once a caller has shown the reference's pattern -- oneRound after oneRound on one
  // unchanged vector -- a call enqueues its own round and up to run_ahead more as ONE graph launch (a hipGraphLaunch of 1..8
  // kernels costs the host 5.5-5.9 us whatever their number, a plain launch 3.0: tools/micro/host_call_cost.hip), and the next
  // calls find their round already in the stream: they only compare.  Round a writes slot a % PICP_SLOTS of the partial rows
  // and of the pose.  The call that enqueues rounds k .. k + run_ahead may still find its OWN comparison differing and must then
  // repeat round k from slot (k - 1) % PICP_SLOTS: so 1 + run_ahead <= PICP_SLOTS - 1 -- the rounds it enqueued never write the
  // slot of the last counted round; later calls, a getter's finishing launch, or a repeat on other pairs / points / parameters
  // read the slot of a round that was claimed, which nothing enqueued after it has written.  Whatever ran ahead and is not
  // claimed by a matching call is overwritten or ignored.  At most run_ahead rounds of GPU time are spent for nothing when
  // the loop ends.
  int ahead = 0;
  int streak = 0;                // consecutive one_round calls that matched their speculation
  int loop_hint = 0;             // rounds the previous run of calls had when a getter closed it: the reference's loop has a fixed
                                 // count (vo_complete.cpp:163: 100), so the last window of a run is cut to what is left of it and
                                 // nothing runs ahead for nothing; a longer run than last time simply goes on in full windows
  int run_ahead = PICP_SLOTS / 2 - 1;   // VO_PICP_RUN_AHEAD (0: every call enqueues exactly its own round; at most PICP_SLOTS - 2).
                                        // Windows of PICP_SLOTS / 2 rounds start at two alternating slots: two graphs per geometry.
  // A window's graph is captured only the third time it is wanted (key -> times wanted): a caller whose correspondence count --
  // and with it the launch geometry -- changes from frame to frame never pays a capture (~0.15 ms each), it gets one plain
  // launch per call as before (apps/one_round_rate, with_init_varying_sizes: 54 k iterations/s with eager captures, 115-120 k
  // without); and nothing is ever destroyed to make room: a full cache means plain launches for new keys.
  std::map<std::tuple<int, int, const void*, size_t, const void*, int>, int> chain_wanted;
  unsigned long long spec_rounds = 0, spec_redone = 0;   // one_round calls enqueued before their comparison / found different
  int use_graph = 1;
  int graph_failures = 0;     // captures that failed (the handle then stays on plain launches): vo_picp_graph_info
  // Which solves take the tail form (picp_tail_policy).  tail_report: PICP_TAIL_REPORT_WORDS ints in pinned host memory that
  // the tail launches of this handle write -- how many of them took the skip path straight, how many ran real rounds inside the
  // launch, the run of skip-path launches with the latest round one of them found its repeat in, the last in-launch round.
  int* tail_report = nullptr;
  int tail_seen[2] = {0, 0};  // the report as last looked at
  int tail_m = PICP_TAIL_FROM;   // the M of the handle's solves in the form: lowered to where its solves repeat, never for a probe
  unsigned long long solves = 0; // solves enqueued (VO_PICP_TAIL_LOG's line says at which of them a graph was captured)
  unsigned long long graph_solves = 0, plain_solves = 0;   // multi-round solves replayed from a graph / submitted plainly: voe_picp_submit_info
  bool plain_logged = false;  // VO_PICP_TAIL_LOG's line for the handle's first tail-form solve submitted plainly has been printed
  bool tail_on = false;       // eligible solves take the form
  bool tail_probe = false;    // one solve in the form is in flight to find out; launches per round until it reports
  int tail_period = PICP_TAIL_PROBE_EVERY, tail_since = PICP_TAIL_PROBE_EVERY - 1;   // off: every tail_period-th eligible solve probes
  std::map<std::tuple<int, int, const void*, size_t, const void*, int>, hipGraphExec_t> graphs;
};

int set_device(vo_ctx* ctx) {
  VO_HIP_CHECK(hipSetDevice(ctx->device));
  return VO_OK;
}

// the `it` argument of round a >= 1 of an open chain (and of the finishing launch after a rounds): only its residue modulo
// PICP_SLOTS matters to the kernels (which slot they read and write), so a chain of any length cycles through 1 .. PICP_SLOTS
static int chain_it(int a) { return a <= 0 ? 0 : ((a - 1) % PICP_SLOTS) + 1; }

// the finishing launch of the rounds vo_picp_one_round has enqueued so far (vo_picp::chain_len), if any
static int picp_flush(vo_picp* s) {
  if (s->chain_len == 0) { s->ahead = 0; return VO_OK; }
  vo_ctx* c = s->ctx;
  if (c->capturing)
    return fail(VO_ERR_NOT_READY, "vo_picp: rounds of vo_picp_one_round are still open (read the pose or the statistics once before the capture)");
  PackedCorr pk{s->packed.as<float>(), s->packed.cap / (5 * sizeof(float)) & ~(size_t)3};
  // (rounds that ran ahead of the caller sit in front of this launch in the stream; they wrote other slots than the one it reads)
  VO_HIP_CHECK(launch_picp_finish(c->stream, s->d_params, s->d_state, pk, s->partials.as<float>(), s->grid, chain_it(s->chain_len)));
  s->loop_hint = s->chain_len;
  s->chain_len = 0;
  s->ahead = 0;
  return VO_OK;
}

extern "C" {

int vo_abi_version(void) { return VO_HIP_ABI_VERSION; }
const char* vo_last_error(void) { return g_err; }

int vo_ctx_create(int device, void* stream, vo_ctx** out) {
  VO_REQUIRE(out != nullptr, "out is null");
  *out = nullptr;
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n <= 0)
    return fail(VO_ERR_NO_DEVICE, "no HIP device available (%s); libvo_hip has no CPU fallback",
                e == hipSuccess ? "count=0" : hipGetErrorString(e));
  if (device < 0 || device >= n) return fail(VO_ERR_INVALID_ARG, "device %d out of range [0,%d)", device, n);
  VO_HIP_CHECK(hipSetDevice(device));
  hipDeviceProp_t prop;
  VO_HIP_CHECK(hipGetDeviceProperties(&prop, device));
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return fail(VO_ERR_NO_DEVICE, "device %d is %s; libvo_hip is built for gfx950 only", device,
                prop.gcnArchName);
  vo_ctx* c = new vo_ctx();
  c->device = device;
  c->n_cu = prop.multiProcessorCount;
  snprintf(c->name, sizeof(c->name), "%s (%s)", prop.name, prop.gcnArchName);
  if (stream) {
    c->stream = reinterpret_cast<hipStream_t>(stream);
  } else {
    hipError_t es = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    if (es != hipSuccess) { delete c; return fail(VO_ERR_HIP, "hipStreamCreate: %s", hipGetErrorString(es)); }
    c->own_stream = true;
  }
  { std::lock_guard<std::mutex> lk(g_ctx_mu); c->id = g_ctx_next_id++; g_ctx_live.insert(c); }
  *out = c;
  return VO_OK;
}

int vo_ctx_destroy(vo_ctx* c) {
  if (!c) return VO_OK;
  {
    std::lock_guard<std::mutex> lk(g_ctx_mu);
    if (!g_ctx_live.erase(c)) return fail(VO_ERR_INVALID_ARG, "vo_ctx_destroy: not a live context (destroyed twice?)");
  }
  (void)hipSetDevice(c->device);
  (void)hipStreamSynchronize(c->stream);
  c->scratch.release(); c->best.release(); c->table.release(); c->counts.release();
  c->batch_pack.release(); c->batch_bad.release(); c->prune_ws.release(); c->epi_ws.release(); c->ransac_ws.release(); c->pose_ws.release();
  c->pose_batch_ws.release(); c->track_ws.release(); c->refine_ws.release(); c->pose_graph_ws.release();
  if (c->hint_ev) (void)hipEventDestroy(c->hint_ev);
  if (c->hint_host) (void)hipHostFree(c->hint_host);
  if (c->hint_dev) (void)hipFree(c->hint_dev); c->batch_states.release(); c->batch_partials.release(); c->batch_help.release();
  for (auto& b : c->in) b.release();
  for (auto& b : c->out) b.release();
  if (c->own_stream) (void)hipStreamDestroy(c->stream);
  delete c;
  return VO_OK;
}

int vo_ctx_synchronize(vo_ctx* c) {
  VO_REQUIRE(c, "ctx is null");
  VO_NOT_CAPTURING(c);
  VO_HIP_CHECK(hipStreamSynchronize(c->stream));
  return VO_OK;
}

void* vo_ctx_stream(vo_ctx* c) { return c ? reinterpret_cast<void*>(c->stream) : nullptr; }
int vo_ctx_device(vo_ctx* c) { return c ? c->device : -1; }
int vo_ctx_capturing(vo_ctx* c) { return (ctx_alive(c) && c->capturing) ? 1 : 0; }
int vo_ctx_alive(vo_ctx* c) { return ctx_alive(c) ? 1 : 0; }
unsigned long long vo_ctx_id(vo_ctx* c) { std::lock_guard<std::mutex> lk(g_ctx_mu); return (c && g_ctx_live.count(c)) ? c->id : 0ull; }

int vo_ctx_device_info(vo_ctx* c, char* name, int name_len, int* n_cu) {
  VO_REQUIRE(c, "ctx is null");
  if (name && name_len > 0) { strncpy(name, c->name, (size_t)name_len - 1); name[name_len - 1] = 0; }
  if (n_cu) *n_cu = c->n_cu;
  return VO_OK;
}

int vo_ctx_begin_capture(vo_ctx* c) {
  VO_REQUIRE(c, "ctx is null");
  VO_REQUIRE(!c->capturing, "already capturing");
  if (int r = set_device(c)) return r;
  VO_HIP_CHECK(hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal));
  c->capturing = true;
  return VO_OK;
}

int vo_ctx_end_capture(vo_ctx* c, vo_graph** out) {
  VO_REQUIRE(c && out, "null argument");
  VO_REQUIRE(c->capturing, "not capturing");
  *out = nullptr;
  c->capturing = false;
  hipGraph_t graph = nullptr;
  hipError_t ee = hipStreamEndCapture(c->stream, &graph);
  if (ee != hipSuccess) {
    // a capture invalidated by a call that cannot be captured: make sure the stream is out of capture mode again
    (void)hipGetLastError();
    if (graph) (void)hipGraphDestroy(graph);
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(c->stream, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone) {
      (void)hipGetLastError();
      if (c->own_stream) {
        hipStream_t fresh = nullptr;
        if (hipStreamCreateWithFlags(&fresh, hipStreamNonBlocking) == hipSuccess) { (void)hipStreamDestroy(c->stream); c->stream = fresh; }
      }
    }
    return fail(VO_ERR_HIP, "hipStreamEndCapture: %s (the captured sequence contained a call that cannot be captured)", hipGetErrorString(ee));
  }
  hipGraphExec_t exec = nullptr;
  hipError_t e = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
  (void)hipGraphDestroy(graph);
  if (e != hipSuccess) { (void)hipGetLastError(); return fail(VO_ERR_HIP, "hipGraphInstantiate: %s", hipGetErrorString(e)); }
  vo_graph* g = new vo_graph();
  g->ctx = c;
  g->ctx_id = c->id;
  g->exec = exec;
  *out = g;
  return VO_OK;
}

int vo_graph_launch(vo_graph* g) {
  VO_REQUIRE(g && g->exec, "null graph");
  VO_REQUIRE(ctx_alive(g->ctx, g->ctx_id), "the context this graph was captured on has been destroyed");
  if (int r = set_device(g->ctx)) return r;
  VO_HIP_CHECK(hipGraphLaunch(g->exec, g->ctx->stream));
  return VO_OK;
}

int vo_graph_destroy(vo_graph* g) {
  if (!g) return VO_OK;
  if (ctx_alive(g->ctx, g->ctx_id)) (void)hipStreamSynchronize(g->ctx->stream);
  else (void)hipDeviceSynchronize();
  if (g->exec) (void)hipGraphExecDestroy(g->exec);
  delete g;
  return VO_OK;
}

// ---- cross-context ordering ------------------------------------------------------------------
int vo_event_create(vo_ctx* c, vo_event** out) {
  VO_REQUIRE(c && out, "null argument");
  *out = nullptr;
  if (int r = set_device(c)) return r;
  hipEvent_t e = nullptr;
  VO_HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  vo_event* v = new vo_event();
  v->device = c->device; v->ev = e;
  *out = v;
  return VO_OK;
}

int vo_event_record(vo_event* ev, vo_ctx* c) {
  VO_REQUIRE(ev && ev->ev && c, "null argument");
  VO_REQUIRE(ev->device == c->device, "event and context live on different devices");
  if (int r = set_device(c)) return r;
  VO_HIP_CHECK(hipEventRecord(ev->ev, c->stream));
  return VO_OK;
}

int vo_ctx_wait_event(vo_ctx* c, vo_event* ev) {
  VO_REQUIRE(ev && ev->ev && c, "null argument");
  VO_REQUIRE(ev->device == c->device, "event and context live on different devices");
  if (int r = set_device(c)) return r;
  VO_HIP_CHECK(hipStreamWaitEvent(c->stream, ev->ev, 0));
  return VO_OK;
}

int vo_event_destroy(vo_event* ev) {
  if (!ev) return VO_OK;
  if (ev->ev) (void)hipEventDestroy(ev->ev);
  delete ev;
  return VO_OK;
}

int vo_dev_alloc(vo_ctx* c, size_t bytes, void** dptr) {
  VO_REQUIRE(c && dptr, "null argument");
  VO_NOT_CAPTURING(c);
  if (int r = set_device(c)) return r;
  VO_HIP_CHECK(hipMalloc(dptr, bytes ? bytes : 16));
  return VO_OK;
}

int vo_dev_free(vo_ctx* c, void* dptr) {
  VO_REQUIRE(c, "ctx is null");
  VO_NOT_CAPTURING(c);
  if (!dptr) return VO_OK;
  VO_HIP_CHECK(hipStreamSynchronize(c->stream));
  VO_HIP_CHECK(hipFree(dptr));
  return VO_OK;
}

int vo_memcpy_h2d(vo_ctx* c, void* dst, const void* src, size_t bytes) {
  VO_REQUIRE(c && (bytes == 0 || (dst && src)), "null argument");
  VO_NOT_CAPTURING(c);
  if (bytes == 0) return VO_OK;
  VO_HIP_CHECK(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, c->stream));
  VO_HIP_CHECK(hipStreamSynchronize(c->stream));
  return VO_OK;
}

int vo_memcpy_d2h(vo_ctx* c, void* dst, const void* src, size_t bytes) {
  VO_REQUIRE(c && (bytes == 0 || (dst && src)), "null argument");
  VO_NOT_CAPTURING(c);
  if (bytes == 0) return VO_OK;
  VO_HIP_CHECK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream));
  VO_HIP_CHECK(hipStreamSynchronize(c->stream));
  return VO_OK;
}

}  // extern "C"

// ---- helpers for the host-pointer entry points ------------------------------------
int upload(vo_ctx* c, DevBuf& b, const void* src, size_t bytes) {
  VO_HIP_CHECK(b.ensure(bytes ? bytes : 16, c->stream));
  if (bytes) VO_HIP_CHECK(hipMemcpyAsync(b.p, src, bytes, hipMemcpyHostToDevice, c->stream));
  return VO_OK;
}

int ensure_counts(vo_ctx* c) {
  VO_HIP_CHECK(c->counts.ensure(64 * sizeof(int), c->stream));
  return VO_OK;
}

static int ensure_scratch(vo_ctx* c, int n) {
  VO_HIP_CHECK(c->scratch.ensure(compaction_scratch_ints(n) * sizeof(int), c->stream));
  return VO_OK;
}

static CamK make_cam(int rows, int cols, int z_near, int z_far, const float K[9]) {
  CamK cam;
  for (int i = 0; i < 9; ++i) cam.K[i] = K[i];
  cam.rows = rows; cam.cols = cols; cam.z_near = z_near; cam.z_far = z_far;
  return cam;
}

extern "C" {

// ---- projectPoints ------------------------------------------------------------------
int vo_project_points_dev(vo_ctx* c, int rows, int cols, int z_near, int z_far, const float K[9],
                          const float T[16], const float* d_world, int n, int keep_indices,
                          float* d_out_uv, int* d_counts) {
  VO_REQUIRE(c && K && T && d_counts, "null argument");
  VO_REQUIRE(n >= 0 && (n == 0 || (d_world && d_out_uv)), "bad point arrays");
  if (int r = set_device(c)) return r;
  if (int r = ensure_scratch(c, n)) return r;
  VO_HIP_CHECK(launch_project_points(c->stream, make_cam(rows, cols, z_near, z_far, K),
                                     pose_from_T16(T), d_world, n, keep_indices, d_out_uv, d_counts,
                                     c->scratch.as<int>()));
  return VO_OK;
}

int vo_project_points(vo_ctx* c, int rows, int cols, int z_near, int z_far, const float K[9],
                      const float T[16], const float* world, int n, int keep_indices, float* out_uv,
                      int* n_out, int* n_inside) {
  VO_REQUIRE(c && K && T, "null argument");
  VO_NOT_CAPTURING(c);
  VO_REQUIRE(n >= 0 && (n == 0 || (world && out_uv)), "bad point arrays");
  if (int r = set_device(c)) return r;
  if (int r = upload(c, c->in[0], world, sizeof(float) * 3 * (size_t)n)) return r;
  VO_HIP_CHECK(c->out[0].ensure(sizeof(float) * 2 * (size_t)(n ? n : 1), c->stream));
  if (int r = ensure_counts(c)) return r;
  if (int r = vo_project_points_dev(c, rows, cols, z_near, z_far, K, T, c->in[0].as<float>(), n,
                                    keep_indices, c->out[0].as<float>(), c->counts.as<int>()))
    return r;
  int h[2] = {0, 0};
  VO_HIP_CHECK(hipMemcpyAsync(h, c->counts.p, sizeof(h), hipMemcpyDeviceToHost, c->stream));
  VO_HIP_CHECK(hipStreamSynchronize(c->stream));
  if (h[0] > 0)
    VO_HIP_CHECK(hipMemcpyAsync(out_uv, c->out[0].p, sizeof(float) * 2 * (size_t)h[0], hipMemcpyDeviceToHost, c->stream));
  VO_HIP_CHECK(hipStreamSynchronize(c->stream));
  if (n_out) *n_out = h[0];
  if (n_inside) *n_inside = h[1];
  return VO_OK;
}

// ---- PICPSolver -----------------------------------------------------------------------
int vo_picp_create(vo_ctx* c, vo_picp** out) {
  VO_REQUIRE(c && out, "null argument");
  VO_NOT_CAPTURING(c);
  *out = nullptr;
  if (int r = set_device(c)) return r;
  vo_picp* s = new vo_picp();
  s->ctx = c;
  s->ctx_id = c->id;
  memset(&s->hp, 0, sizeof(s->hp));
  const float I3[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
  s->hp.cam = make_cam(100, 100, 0, 10, I3);     // Camera defaults, camera.h:16-21
  s->hp.thr = 1000.f;                            // picp_solver.cpp:13
  s->hp.damping = 1.f;                           // picp_solver.cpp:10
  s->hp.keep_outliers = 0;
  s->hp.n_corr = 0;
  const char* g = getenv("VO_PICP_GRAPH");
  if (g) s->use_graph = atoi(g);
  if (const char* ra = getenv("VO_PICP_RUN_AHEAD")) { const int v = atoi(ra); s->run_ahead = v < 0 ? 0 : (v > PICP_SLOTS - 2 ? PICP_SLOTS - 2 : v); }
  hipError_t e = hipMalloc(reinterpret_cast<void**>(&s->d_params), sizeof(PicpParams));
  if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&s->d_state), sizeof(PicpState));
  if (e == hipSuccess) e = hipMemsetAsync(s->d_state, 0, sizeof(PicpState), c->stream);
  // (without the report the handle keeps a launch per round: picp_tail_policy)
  if (e == hipSuccess && hipHostMalloc(reinterpret_cast<void**>(&s->tail_report), PICP_TAIL_REPORT_WORDS * sizeof(int), hipHostMallocDefault) == hipSuccess) {
    for (int k = 0; k < PICP_TAIL_REPORT_WORDS; ++k) s->tail_report[k] = 0;
  } else if (e == hipSuccess) {
    (void)hipGetLastError();
    s->tail_report = nullptr;
  }
  if (e != hipSuccess) {
    if (s->d_params) (void)hipFree(s->d_params);
    if (s->d_state) (void)hipFree(s->d_state);
    if (s->tail_report) (void)hipHostFree(s->tail_report);
    delete s;
    return fail(VO_ERR_HIP, "vo_picp_create: %s", hipGetErrorString(e));
  }
  // identity pose
  float pose[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0};
  VO_HIP_CHECK(hipMemcpyAsync(s->d_state->pose[0], pose, sizeof(pose), hipMemcpyHostToDevice, c->stream));
  VO_HIP_CHECK(hipStreamSynchronize(c->stream));
  *out = s;
  return VO_OK;
}

int vo_picp_destroy(vo_picp* s) {
  if (!s) return VO_OK;
  if (ctx_alive(s->ctx, s->ctx_id)) {
    VO_NOT_CAPTURING(s->ctx);
    (void)hipSetDevice(s->ctx->device);
    (void)hipStreamSynchronize(s->ctx->stream);
  } else {
    (void)hipDeviceSynchronize();       // the context went first: its stream is gone, the solver's memory is not
  }
  for (auto& kv : s->graphs) (void)hipGraphExecDestroy(kv.second);
  s->world_own.release(); s->meas_own.release(); s->pairs_own.release();
  s->packed.release(); s->partials.release();
  if (s->d_params) (void)hipFree(s->d_params);
  if (s->d_state) (void)hipFree(s->d_state);
  if (s->tail_report) (void)hipHostFree(s->tail_report);
  delete s;
  return VO_OK;
}

int vo_picp_set_pose(vo_picp* s, const float T[16]) {
  VO_REQUIRE(s && T, "null argument");
  VO_REQUIRE(ctx_alive(s->ctx, s->ctx_id), "the context this solver was made on has been destroyed");
  VO_NOT_CAPTURING(s->ctx);
  if (int r = set_device(s->ctx)) return r;
  const Pose P = pose_from_T16(T);
  float pose[12];
  for (int i = 0; i < 9; ++i) pose[i] = P.R[i];
  for (int i = 0; i < 3; ++i) pose[9 + i] = P.t[i];
  s->pending_T0 = nullptr;
  if (int r = picp_flush(s)) return r;     // open rounds first: H, b and the statistics stay those of the last round
  VO_HIP_CHECK(hipMemcpyAsync(s->d_state->pose[0], pose, sizeof(pose), hipMemcpyHostToDevice,
                              s->ctx->stream));
  VO_HIP_CHECK(hipStreamSynchronize(s->ctx->stream));   // `pose` is a stack buffer
  return VO_OK;
}

int vo_picp_set_camera(vo_picp* s, int rows, int cols, int z_near, int z_far, const float K[9],
                       const float T[16]) {
  VO_REQUIRE(s && K && T, "null argument");
  VO_REQUIRE(ctx_alive(s->ctx, s->ctx_id), "the context this solver was made on has been destroyed");
  s->hp.cam = make_cam(rows, cols, z_near, z_far, K);
  s->params_dirty = true;
  return vo_picp_set_pose(s, T);
}

int vo_picp_set_kernel_threshold(vo_picp* s, float thr) {
  VO_REQUIRE(s, "null argument");
  VO_REQUIRE(ctx_alive(s->ctx, s->ctx_id), "the context this solver was made on has been destroyed");
  s->hp.thr = thr;
  s->params_dirty = true;
  return VO_OK;
}

void picp_set_camera_threshold(vo_picp* s, int rows, int cols, int z_near, int z_far, const float K[9], float thr) {
  const CamK cam = make_cam(rows, cols, z_near, z_far, K);
  if (memcmp(&cam, &s->hp.cam, sizeof(cam)) != 0) { s->hp.cam = cam; s->params_dirty = true; }
  if (memcmp(&thr, &s->hp.thr, sizeof(thr)) != 0) { s->hp.thr = thr; s->params_dirty = true; }
}
const PicpState* picp_state_dev(const vo_picp* s) { return s->d_state; }

int vo_picp_get_kernel_threshold(vo_picp* s, float* thr) {
  VO_REQUIRE(s && thr, "null argument");
  VO_REQUIRE(ctx_alive(s->ctx, s->ctx_id), "the context this solver was made on has been destroyed");
  *thr = s->hp.thr;
  return VO_OK;
}

int vo_picp_set_points_dev(vo_picp* s, const float* d_world, int n_world, const float* d_meas, int n_meas) {
  VO_REQUIRE(s, "null argument");
  VO_REQUIRE(ctx_alive(s->ctx, s->ctx_id), "the context this solver was made on has been destroyed");
  VO_REQUIRE(n_world >= 0 && n_meas >= 0, "negative count");
  VO_REQUIRE((n_world == 0 || d_world) && (n_meas == 0 || d_meas), "null point array");
  s->d_world = d_world; s->n_world = n_world;
  s->d_meas = d_meas; s->n_meas = n_meas;
  s->have_points = true;
  s->packed_valid = false;
  return VO_OK;
}

int vo_picp_set_points(vo_picp* s, const float* world, int n_world, const float* meas, int n_meas) {
  VO_REQUIRE(s, "null argument");
  VO_REQUIRE(ctx_alive(s->ctx, s->ctx_id), "the context this solver was made on has been destroyed");
  VO_NOT_CAPTURING(s->ctx);
  VO_REQUIRE(n_world >= 0 && n_meas >= 0, "negative count");
  VO_REQUIRE((n_world == 0 || world) && (n_meas == 0 || meas), "null point array");
  if (int r = set_device(s->ctx)) return r;
  if (int r = upload(s->ctx, s->world_own, world, sizeof(float) * 3 * (size_t)n_world)) return r;
  if (int r = upload(s->ctx, s->meas_own, meas, sizeof(float) * 2 * (size_t)n_meas)) return r;
  VO_HIP_CHECK(hipStreamSynchronize(s->ctx->stream));
  return vo_picp_set_points_dev(s, s->world_own.as<float>(), n_world, s->meas_own.as<float>(), n_meas);
}

}  // extern "C"

__global__ void T16_to_pose12_kernel(const float* T, float* p) {
  const int k = threadIdx.x;
  if (k < 9) p[k] = T[(k % 3) + 4 * (k / 3)];
  else if (k < 12) p[k] = T[12 + (k - 9)];
}

static bool picp_chainable(const vo_picp* s);

// VO_PICP_GATHER=0 in the environment keeps the separate gather launch in front of every solve (read per call: tests compare
// the two routes in one process)
static bool picp_gather_enabled() { const char* e = getenv("VO_PICP_GATHER"); return !(e && e[0] == '0'); }
// VO_PICP_CYCLE=0 in the environment turns the cycle detection of a launch-per-round solve off (read per call, part of the
// graph's key): no detector workgroup, every round runs.  Diagnostic runs of the round itself (stamps, step splits) set it.
static bool picp_cycle_enabled() { const char* e = getenv("VO_PICP_CYCLE"); return !(e && e[0] == '0'); }

// Which solves take the tail form (picp.hip, picp_tail_kernel).  The form wins 1.7 us for every launch that would only return
// -- half of the 50-round headline step -- where the pose repeats within the first PICP_TAIL_FROM rounds, and loses ~10 us for
// every round that has to run inside the launch where it does not (the sequence leg's frames never repeat in 100 rounds:
// DESIGN.md section 4.1).  Which of the two a caller's problems are is only known afterwards, and the host must not wait for
// the device to find out.  So every tail launch reports how it went into two host-visible counters (PicpTailTally), and an
// enqueue looks at whatever has arrived by then:
//   * a handle starts with ONE solve in the form, a probe; until it has reported, solves keep a launch per round;
//   * a probe that took the skip path switches the form on; a tail launch that ran real rounds switches it off;
//   * while off, one eligible solve in tail_period is a probe; the period doubles with every probe that ran real rounds.
// A caller that runs far ahead of the device therefore pays for at most one slow solve per probe, never for a queue of them.
// Results are the same bytes in either form, so the choice is invisible but for the time.  An explicit VO_PICP_TAIL=1 or
// VO_PICP_TAIL_FROM takes the form for every eligible solve (tests, measurements); solves captured into a caller's graph keep
// a launch per round (the choice would be frozen into the graph).
//
// Where the tail launch starts.  Every launch between the one that found the repeat and M is a bare kernel boundary (1.72 us),
// so a handle whose solves keep repeating early is better off with a lower M.  The tail launches report the run of consecutive
// skip-path launches and the largest detected_at among them (one word: never a torn pair); once the run is at least
// PICP_TAIL_LEARN the handle's M is min(PICP_TAIL_FROM, largest detected_at + 1).  The margin of one round: a solve that
// repeats one round later than any of the last eight still finds its repeat in a launch of its own and takes the skip path.
// A miss costs ~10 us per round run in the launch, a hit saves 1.72 us per spared launch -- one missed round eats the gain of
// six spared launches, hence eight witnesses and the margin rather than the latest solve's value.  A launch at a lowered M that
// ran real rounds puts M back to PICP_TAIL_FROM and the device starts the run again; the form goes off only where the last
// in-launch round lay beyond PICP_TAIL_FROM, i.e. where a tail at the default M would have looped as well.  M is never
// lowered for a probe, and eligibility is judged with the M chosen.  Graphs are keyed by M; none of this waits for the device.
//
// The early form (picp.hip, picp_tail_kernel<.., EARLY>) is a further tier on top of the learned M: its tail launch is the one
// that COMPUTES the repeating pose and closes the solve in the same round, so it starts at M = largest detected_at - 2 -- no
// margin round, and no launch that only finds out.  A solve that repeats earlier is caught by an ordinary detector and closes
// from the ring at the start as ever; one that repeats later runs real rounds inside the launch, and the rule above applies: M
// back to PICP_TAIL_FROM, the run starts again.  Without a margin a miss is likelier, so the tier asks for
// PICP_TAIL_EARLY_LEARN witnesses.  An early close counts as a skip-path launch in the report.  VO_PICP_TAIL_EARLY=0 keeps the
// host from choosing the form, VO_PICP_TAIL_EARLY=1 adds it to a forced M (read per call; *early is part of the graph's key).
//
// How the solve is submitted (*plain: plain launches throughout, no graph).  A replayed graph costs the device time around
// it that plain launches of the same kernels do not: at 50 000 pairs the headline step is 47.6 us behind round 0 + graph and
// 41.7 us as eleven plain launches (medians of five, alternating; ranges 47.5-48.2 against 40.6-42.3), the learned ring form
// at M = 12 55.4 against 52.5 (55.0-55.9 against 49.1-52.7); eleven do-nothing kernels of a round's length take 53.7 us per
// step behind a graph and 50.3 us plainly (tools/micro/step_gap): profiles/step_gap.json, DESIGN.md section 8 "Between two
// steps".  The price is host time: eleven plain launches take the host 31 us where round 0 and a graph launch of ten kernels
// take 9, so a plain solve stays ahead of the device only while its launches are real rounds (3.45 us each; an empty kernel
// takes the device 2.2 us, less than the 2.8 us the host needs to launch it).  That is what a learned M
// says of a handle -- its witnesses found every launch up to M at work --, so the early tier and the learned ring tier
// (tail_m < PICP_TAIL_FROM) go plain; probes, skip-path solves at the default M (whose launches 12 .. 16 return in 1.72 us,
// faster than the host issues them) and every solve without a tail form keep the graph, and so does a forced M, so that a
// test of the forms runs the path it ran.  VO_PICP_TAIL_SUBMIT=graph|plain (read per call) forces the form for every
// tail-form solve, a forced M included.  Same kernels, same arguments, same bytes either way.
static int picp_tail_submit_env() { const char* e = getenv("VO_PICP_TAIL_SUBMIT"); return !e ? -1 : (e[0] == 'p' ? 1 : (e[0] == 'g' ? 0 : -1)); }

static int picp_tail_policy(vo_picp* s, int n_iters, bool cycle, bool* early, bool* plain) {
  bool forced = false;
  *early = false;
  *plain = false;
  const int early_env = picp_tail_early_env();
  const int submit_env = picp_tail_submit_env();
  const int m = picp_tail_from(s->grid, n_iters, cycle, s->ctx->n_cu, &forced);
  if (forced) { *early = m > 0 && early_env == 1; *plain = m > 0 && submit_env == 1; return m; }
  // (not eligible at the default M and the form not on: no M this handle may choose would make it eligible -- nothing to look at)
  if (m == 0 && !s->tail_on) return 0;
  if (!cycle || s->ctx->capturing || !s->tail_report) return 0;
  if (const char* e = getenv("VO_PICP_TAIL")) if (e[0] == '0') return 0;
  // ([1] before [3] before [2]: behind a launch that ran real rounds the device stores them the other way round)
  int now[2];
  now[1] = __atomic_load_n(&s->tail_report[1], __ATOMIC_ACQUIRE);
  const int last_round_word = __atomic_load_n(&s->tail_report[3], __ATOMIC_ACQUIRE);
  const int run_word = __atomic_load_n(&s->tail_report[2], __ATOMIC_ACQUIRE);
  now[0] = __atomic_load_n(&s->tail_report[0], __ATOMIC_RELAXED);
  const bool straight = now[0] != s->tail_seen[0], looped = now[1] != s->tail_seen[1];
  s->tail_seen[0] = now[0];
  s->tail_seen[1] = now[1];
  // the last round the latest looping launch ran; unknown (the tag is another launch's) counts as beyond the default M
  const bool tagged = ((last_round_word >> 16) & 0xffff) == (now[1] & 0xffff);
  const int last_round = tagged ? (last_round_word & 0xffff) : 0xffff;
  if (looped && s->tail_on && last_round <= PICP_TAIL_FROM) {
    s->tail_m = PICP_TAIL_FROM;         // a lowered M missed a repeat the default M would have caught: the form stays on
  } else if (looped) {
    s->tail_period = s->tail_probe ? (s->tail_period < PICP_TAIL_PROBE_MAX ? 2 * s->tail_period : PICP_TAIL_PROBE_MAX) : PICP_TAIL_PROBE_EVERY;
    s->tail_on = false;
    s->tail_probe = false;
    s->tail_since = 0;
    s->tail_m = PICP_TAIL_FROM;
  } else if (straight && s->tail_probe) {
    s->tail_on = true;
    s->tail_probe = false;
    s->tail_period = PICP_TAIL_PROBE_EVERY;
  }
  if (s->tail_on) {
    if (!looped) {
      const int run = (run_word >> 16) & 0xffff, det = run_word & 0xffff;
      if (run >= PICP_TAIL_LEARN && det >= 1) s->tail_m = det + 1 < PICP_TAIL_FROM ? det + 1 : PICP_TAIL_FROM;
      if (early_env != 0 && run >= PICP_TAIL_EARLY_LEARN && det >= 3) {
        const int me = picp_tail_from(s->grid, n_iters, cycle, s->ctx->n_cu, nullptr, det - 2 < PICP_TAIL_FROM ? det - 2 : PICP_TAIL_FROM);
        if (me > 0) { *early = true; *plain = submit_env != 0; return me; }
      }
    }
    const int ml = picp_tail_from(s->grid, n_iters, cycle, s->ctx->n_cu, nullptr, s->tail_m);
    *plain = ml > 0 && (s->tail_m < PICP_TAIL_FROM ? submit_env != 0 : submit_env == 1);
    return ml;
  }
  if (s->tail_probe || m == 0) return 0;
  if (++s->tail_since < s->tail_period) return 0;
  s->tail_since = 0;
  s->tail_probe = true;
  *plain = submit_env == 1;
  return m;
}

// n_iters / lazy: what the caller hands to picp_enqueue next (0: nothing that could take the gather along)
static int picp_prepare(vo_picp* s, const int32_t* d_pairs, int n_pairs, const int* d_n, int keep_outliers, int n_iters = 0,
                        bool lazy = false) {
  vo_ctx* c = s->ctx;
  if (!s->have_points) return fail(VO_ERR_NOT_READY, "vo_picp: set_points has not been called");
  if (s->hp.keep_outliers != (keep_outliers ? 1 : 0)) { s->hp.keep_outliers = keep_outliers ? 1 : 0; s->params_dirty = true; }
  if (s->params_dirty && c->capturing)
    return fail(VO_ERR_NOT_READY, "vo_picp: parameters changed inside a graph capture (run the sequence once before capturing)");
  if (s->params_dirty) {
    // n_corr is owned by the pack kernel: keep the device value
    VO_HIP_CHECK(hipMemcpyAsync(s->d_params, &s->hp, offsetof(PicpParams, n_corr), hipMemcpyHostToDevice,
                                c->stream));
    VO_HIP_CHECK(hipStreamSynchronize(c->stream));
    s->params_dirty = false;
  }
  if (!s->packed_valid) {
    const size_t cap = ((size_t)(n_pairs > 0 ? n_pairs : 1) + 3) & ~(size_t)3;
    VO_HIP_CHECK(s->packed.ensure(sizeof(float) * 5 * cap, c->stream));
    {
      // open rounds read the partial rows of their predecessor at the chain's grid: another grid closes the chain first
      const int g = picp_grid_for(n_pairs, c->n_cu);
      if (g != s->grid) { if (int r = picp_flush(s)) return r; }
      s->grid = g;
    }
    {
      // two buffers of round_up(grid,256) rows; rows >= grid are never written and must read as zero
      const size_t rows = ((size_t)s->grid + 255) & ~(size_t)255;
      const size_t bytes = sizeof(float) * PICP_SLOTS * rows * PICP_PSTRIDE * PICP_REPLICAS;
      if (bytes > s->partials.cap || s->grid != s->zeroed_for_grid) {
        VO_HIP_CHECK(s->partials.ensure(bytes, c->stream));
        VO_HIP_CHECK(hipMemsetAsync(s->partials.p, 0, s->partials.cap, c->stream));
        s->zeroed_for_grid = s->grid;
      }
    }
    PackedCorr pk{s->packed.as<float>(), s->packed.cap / (5 * sizeof(float)) & ~(size_t)3};
    // With rounds behind it the gather rides in round 0.  Not where no round kernel follows: the reference-order mode, a
    // single workgroup's all-rounds launch, no round at all, and the one open round of vo_picp_one_round (whose chain
    // kernels are the plain ones).
    if (n_iters >= 1 && !s->exact && picp_rounds_chain(s->grid) && !(lazy && n_iters == 1 && picp_chainable(s)) &&
        picp_gather_enabled()) {
      s->gather = PicpGather{d_pairs, d_n, n_pairs, s->d_world, s->n_world, s->d_meas, s->n_meas, s->pending_T0, 1};
    } else {
      VO_HIP_CHECK(launch_picp_pack(c->stream, d_pairs, d_n, n_pairs, s->d_world, s->n_world, s->d_meas,
                                    s->n_meas, pk, s->d_params, s->d_state, s->pending_T0));
    }
    s->pending_T0 = nullptr;
    s->packed_valid = true;
  }
  if (s->pending_T0) {   // correspondences were cached: the pose reset needs its own (tiny) launch
    hipLaunchKernelGGL(T16_to_pose12_kernel, dim3(1), dim3(64), 0, c->stream, s->pending_T0, s->d_state->pose[0]);
    VO_HIP_CHECK(hipGetLastError());
    s->pending_T0 = nullptr;
  }
  return VO_OK;
}

static bool picp_chainable(const vo_picp* s) { return !s->exact && !s->ctx->capturing && picp_rounds_chain(s->grid); }

// rounds chain_len .. chain_len + n - 1 of the open chain; `count` = false: speculative launches the caller may have to
// repeat or will claim one by one (vo_picp_solve).  n > 1: one graph launch (captured once per starting slot and n).
static int picp_enqueue_chain_rounds(vo_picp* s, int n, bool count) {
  vo_ctx* c = s->ctx;
  PackedCorr pk{s->packed.as<float>(), s->packed.cap / (5 * sizeof(float)) & ~(size_t)3};
  float* partials = s->partials.as<float>();
  const bool pinhole = is_pinhole(s->hp.cam.K), keep = s->hp.keep_outliers != 0;
  const int first = s->chain_len;
  bool done = false;
  if (n > 1 && s->use_graph && first > 0) {
    static_assert(PICP_SLOTS < 64, "key of a window's graph: 64 * rounds + starting slot");
    auto key = std::make_tuple(-(64 * n + chain_it(first)), s->grid, (const void*)pk.base, pk.cap, (const void*)partials,
                               (pinhole ? 1 : 0) | (keep ? 2 : 0));
    auto it = s->graphs.find(key);
    if (it == s->graphs.end() && (s->graphs.size() >= 64 || (s->chain_wanted.size() < 4096 ? ++s->chain_wanted[key] : 3) < 3)) {
      n = 1;                                     // not (yet) worth a capture: this call's own round, plainly
    } else if (it == s->graphs.end()) {
      hipGraph_t graph = nullptr;
      hipGraphExec_t exec = nullptr;
      hipError_t e = hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal);
      if (e == hipSuccess) {
        hipError_t el = hipSuccess;
        for (int k = 0; k < n && el == hipSuccess; ++k)
          el = launch_picp_chain_round(c->stream, s->d_params, s->d_state, pk, partials, s->grid, chain_it(first + k), pinhole, keep);
        e = hipStreamEndCapture(c->stream, &graph);
        if (e == hipSuccess && el != hipSuccess) e = el;
      }
      if (e == hipSuccess) e = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
      if (graph) (void)hipGraphDestroy(graph);
      if (e != hipSuccess) {
        (void)hipGetLastError();
        s->run_ahead = 0;                        // plain launches, one per call, from here on
        ++s->graph_failures;
        (void)fail(VO_OK, "vo_picp: graph capture of %d rounds ahead failed (%s); this solver enqueues one round per call", n, hipGetErrorString(e));
        n = 1;
      } else {
        it = s->graphs.emplace(key, exec).first;
      }
    }
    if (n > 1 && it != s->graphs.end()) {
      VO_HIP_CHECK(hipGraphLaunch(it->second, c->stream));
      done = true;
    }
  }
  if (!done) {
    if (!(s->use_graph && first > 0)) n = 1;     // (the first round of a chain is the kernel without the look at its predecessor)
    for (int k = 0; k < n; ++k)
      VO_HIP_CHECK(launch_picp_chain_round(c->stream, s->d_params, s->d_state, pk, partials, s->grid, chain_it(first + k), pinhole, keep));
  }
  if (count) s->chain_len += n;
  return n;                                      // rounds enqueued (>= 1); errors return through VO_HIP_CHECK as negative codes
}

// lazy: a single round may stay open (no finishing launch) -- host entry points only, whose getters close it
static int picp_enqueue(vo_picp* s, int n_iters, bool lazy = false) {
  vo_ctx* c = s->ctx;
  s->ahead = 0;                                  // whatever ran ahead of the caller is not claimed by this call
  if (lazy && n_iters == 1 && picp_chainable(s)) { const int r = picp_enqueue_chain_rounds(s, 1, true); return r < 0 ? r : VO_OK; }
  const PicpGather gather = s->gather;           // round 0 gathers (picp_prepare) or takes the packed arrays as they are
  s->gather = PicpGather{};
  if (n_iters > 0) { if (int r = picp_flush(s)) { if (gather.on) s->packed_valid = false; return r; } }
  PackedCorr pk{s->packed.as<float>(), s->packed.cap / (5 * sizeof(float)) & ~(size_t)3};
  float* partials = s->partials.as<float>();
  const bool pinhole = is_pinhole(s->hp.cam.K), keep = s->hp.keep_outliers != 0;
  const bool cycle = picp_cycle_enabled();
  if (gather.on && (s->exact || n_iters < 1)) {
    s->packed_valid = false;
    return fail(VO_ERR_NOT_READY, "vo_picp: a gather was left without its round");
  }
  if (s->exact) {
    VO_HIP_CHECK(launch_picp_exact(c->stream, s->d_params, s->d_state, pk, n_iters));
    return VO_OK;
  }
  // rounds behind this index share one launch (0: every round has its own); part of the graph's key
  bool tail_early = false, tail_plain = false;
  const int tail_from = picp_tail_policy(s, n_iters, cycle, &tail_early, &tail_plain);
  // (VO_PICP_TAIL_RING=0, read per call: the tail launch recomputes the last round's rows where the ring holds them)
  const bool tail_ring = tail_from == 0 || picp_tail_ring_enabled();
  ++s->solves;
  if (s->use_graph && n_iters >= 2 && !c->capturing && !tail_plain) {
    // Where the rounds are launches of their own, round 0 -- whose arguments (what it gathers from, or that it does not) are
    // the caller's and change from call to call -- is a plain launch, and the graph holds what follows it: one graph per
    // solve shape, whatever it is replayed behind.  (Round 0 as the graph's first node measured the same: DESIGN.md section 8.)
    const int part = picp_rounds_chain(s->grid) ? PICP_AFTER_ROUND0 : PICP_WHOLE;
    auto key = std::make_tuple(n_iters, s->grid, (const void*)pk.base, pk.cap, (const void*)partials,
                               (pinhole ? 1 : 0) | (keep ? 2 : 0) | (cycle ? 4 : 0) | (tail_ring ? 0 : 8) | (tail_early ? 16 : 0) | (tail_from << 5));
    auto it = s->graphs.find(key);
    if (it == s->graphs.end()) {
      hipGraph_t graph = nullptr;
      hipGraphExec_t exec = nullptr;
      hipError_t e = hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal);
      if (e == hipSuccess) {
        hipError_t el = launch_picp_rounds(c->stream, s->d_params, s->d_state, pk, partials, s->grid, n_iters, pinhole, keep, gather, part, cycle, tail_from, s->tail_report, tail_ring, tail_early);
        e = hipStreamEndCapture(c->stream, &graph);
        if (e == hipSuccess && el != hipSuccess) e = el;
      }
      if (e == hipSuccess) e = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
      if (graph) (void)hipGraphDestroy(graph);
      if (e != hipSuccess) {
        (void)hipGetLastError();
        // The rounds still run, as plain launches (same kernels, same results, ~10 % slower per round at 50k), for the rest
        // of this handle's life -- but not silently: the reason is left in vo_last_error() once and counted, so that a host
        // program (or tests/test_gpu_more.py) can see that its solver lost the graph path.
        s->use_graph = 0;
        ++s->graph_failures;
        (void)fail(VO_OK, "vo_picp: graph capture of %d rounds failed (%s); this solver now uses plain launches", n_iters,
                   hipGetErrorString(e));
      } else {
        if (s->graphs.size() >= 64) {            // (a handle used at ever new sizes: start over -- once nothing of it is in flight)
          (void)hipStreamSynchronize(c->stream);
          for (auto& kv : s->graphs) (void)hipGraphExecDestroy(kv.second);
          s->graphs.clear();
          s->chain_wanted.clear();
        }
        it = s->graphs.emplace(key, exec).first;
        // VO_PICP_TAIL_LOG=1: which solve of the handle paid for a capture, and of which form (stderr; a measurement checks
        // with it that the graph of a learned M is captured inside its warm-up)
        if (const char* lg = getenv("VO_PICP_TAIL_LOG")) if (lg[0] == '1')
          fprintf(stderr, "vo_picp: graph of %d rounds, tail_from %d%s, captured at solve %llu of the handle\n", n_iters, tail_from,
                  tail_early ? " (early form)" : "", s->solves);
      }
    }
    if (s->use_graph && it != s->graphs.end()) {
      hipError_t e = hipSuccess;
      if (part == PICP_AFTER_ROUND0)
        e = launch_picp_rounds(c->stream, s->d_params, s->d_state, pk, partials, s->grid, n_iters, pinhole, keep, gather, PICP_ROUND0, cycle, tail_from, s->tail_report, tail_ring, tail_early);
      if (e == hipSuccess) e = hipGraphLaunch(it->second, c->stream);
      if (e != hipSuccess && gather.on) s->packed_valid = false;
      VO_HIP_CHECK(e);
      ++s->graph_solves;
      return VO_OK;
    }
  }
  {
    // plain launches throughout: a tail-form solve the policy submits so (no graph is captured or looked up for it), a handle
    // without the graph, a single round, a caller's capture
    if (tail_plain && !s->plain_logged) {
      s->plain_logged = true;
      if (const char* lg = getenv("VO_PICP_TAIL_LOG")) if (lg[0] == '1')
        fprintf(stderr, "vo_picp: solve %llu of the handle is its first submitted as plain launches: %d rounds, tail_from %d%s\n", s->solves,
                n_iters, tail_from, tail_early ? " (early form)" : "");
    }
    const hipError_t e = launch_picp_rounds(c->stream, s->d_params, s->d_state, pk, partials, s->grid, n_iters, pinhole, keep, gather,
                                            PICP_WHOLE, cycle, tail_from, s->tail_report, tail_ring, tail_early);
    if (e != hipSuccess && gather.on) s->packed_valid = false;
    VO_HIP_CHECK(e);
    if (n_iters >= 2 && !c->capturing) ++s->plain_solves;
  }
  return VO_OK;
}

extern "C" {

int vo_picp_solve_dev(vo_picp* s, const int32_t* d_pairs, int n_pairs, const int* d_n_pairs,
                      int keep_outliers, int n_iters) {
  VO_REQUIRE(s, "null argument");
  VO_REQUIRE(ctx_alive(s->ctx, s->ctx_id), "the context this solver was made on has been destroyed");
  VO_REQUIRE(n_pairs >= 0 && (n_pairs == 0 || d_pairs), "bad pairs");
  VO_REQUIRE(n_iters >= 0, "negative n_iters");
  if (int r = set_device(s->ctx)) return r;
  if (int r = picp_flush(s)) return r;     // rounds left open by vo_picp_one_round: closed before this solve's launches
  // device pairs may have been rewritten in place by the producer: always re-pack
  s->packed_valid = false;
  s->shadow_valid = false;
  if (int r = picp_prepare(s, d_pairs, n_pairs, d_n_pairs, keep_outliers, n_iters)) return r;
  return picp_enqueue(s, n_iters);
}

// Uploads `pairs` unless the whole array equals what is already packed.  The reference reads the vector on every
// call (picp_solver.cpp:62): an in-place edit between two rounds must be seen, so the comparison covers every
// pair (memcmp against a host copy: ~15 us at 50k pairs, no stream synchronisation when nothing changed).
static int picp_take_pairs(vo_picp* s, const int32_t* pairs, int n_pairs) {
  vo_ctx* c = s->ctx;
  const size_t words = 2 * (size_t)n_pairs;
  const bool same = s->packed_valid && s->shadow_valid && s->shadow.size() == words &&
                    (words == 0 || memcmp(s->shadow.data(), pairs, sizeof(int32_t) * words) == 0);
  if (same) return VO_OK;
  s->shadow_valid = false;
  s->shadow.assign(pairs, pairs + words);
  if (int r = upload(c, s->pairs_own, s->shadow.data(), sizeof(int32_t) * words)) return r;
  VO_HIP_CHECK(hipStreamSynchronize(c->stream));
  s->packed_valid = false;
  s->shadow_valid = true;
  return VO_OK;
}

int vo_picp_solve(vo_picp* s, const int32_t* pairs, int n_pairs, int keep_outliers, int n_iters) {
  VO_REQUIRE(s, "null argument");
  VO_REQUIRE(ctx_alive(s->ctx, s->ctx_id), "the context this solver was made on has been destroyed");
  VO_NOT_CAPTURING(s->ctx);
  VO_REQUIRE(n_pairs >= 0 && (n_pairs == 0 || pairs), "bad pairs");
  VO_REQUIRE(n_iters >= 0, "negative n_iters");
  if (int r = set_device(s->ctx)) return r;
  // ONE round on an array that is probably the one already packed -- the reference's own loop, vo_complete.cpp:163-164:
  // a hundred oneRound calls on one vector -- is enqueued BEFORE the comparison, which then runs while the GPU works.
  // Should the array differ after all, the new pairs are uploaded and packed and the SAME round is enqueued again: the
  // speculative launch has written nothing but the partial rows and the pose slot of its own round index (from the state
  // its predecessor left, which it does not touch), and the repeat overwrites both.
  const size_t words = 2 * (size_t)n_pairs;
  if (n_iters == 1 && s->packed_valid && s->shadow_valid && s->shadow.size() == words && s->have_points &&
      s->hp.keep_outliers == (keep_outliers ? 1 : 0) && !s->params_dirty && picp_chainable(s)) {
    if (int r = picp_prepare(s, s->pairs_own.as<int32_t>(), n_pairs, nullptr, keep_outliers)) return r;   // (a pending pose only)
    int enq = 0;                                 // rounds this call put into the stream (0: its round ran ahead of it)
    if (s->ahead == 0) {
      // the caller has shown the loop (two calls in a row matched): this round and run_ahead more, one graph launch
      int want = s->streak >= 2 ? 1 + s->run_ahead : 1;
      if (s->loop_hint > s->chain_len && want > s->loop_hint - s->chain_len) want = s->loop_hint - s->chain_len;
      enq = picp_enqueue_chain_rounds(s, want, false);
      if (enq < 0) return enq;
    }
    ++s->spec_rounds;
    // (glibc's memcmp runs this pass at the L2 bandwidth of the host core -- 3.5 us for 2 x 400 KB on the EPYC 9575F of the
    // GPU box, faster than a hand-unrolled AVX2 pass: tools/micro/host_call_cost.hip)
    if (words == 0 || memcmp(s->shadow.data(), pairs, sizeof(int32_t) * words) == 0) {
      ++s->chain_len;
      if (enq > 0) s->ahead = enq - 1; else --s->ahead;
      ++s->streak;
      s->set_n = n_pairs;
      return VO_OK;
    }
    ++s->spec_redone;
  }
  s->ahead = 0;                                  // rounds that ran ahead (if any) are not this call's: round chain_len is enqueued again below
  s->streak = 0;
  if (int r = picp_take_pairs(s, pairs, n_pairs)) return r;
  // pairs_own / shadow now hold THIS array: a later vo_picp_rounds continues on it (not on a stale count from an earlier
  // vo_picp_set_correspondences, which would re-pack a mix of both arrays once set_points invalidated the packing)
  s->set_n = n_pairs;
  if (int r = picp_prepare(s, s->pairs_own.as<int32_t>(), n_pairs, nullptr, keep_outliers, n_iters, true)) return r;
  return picp_enqueue(s, n_iters, true);
}

int vo_picp_one_round(vo_picp* s, const int32_t* pairs, int n_pairs, int keep_outliers) {
  return vo_picp_solve(s, pairs, n_pairs, keep_outliers, 1);
}

int vo_picp_set_correspondences(vo_picp* s, const int32_t* pairs, int n_pairs) {
  VO_REQUIRE(s, "null argument");
  VO_REQUIRE(ctx_alive(s->ctx, s->ctx_id), "the context this solver was made on has been destroyed");
  VO_NOT_CAPTURING(s->ctx);
  VO_REQUIRE(n_pairs >= 0 && (n_pairs == 0 || pairs), "bad pairs");
  if (int r = set_device(s->ctx)) return r;
  s->packed_valid = false;          // explicit hand-over: always uploaded
  s->shadow_valid = false;
  if (int r = picp_take_pairs(s, pairs, n_pairs)) return r;
  s->set_n = n_pairs;
  return VO_OK;
}

int vo_picp_rounds(vo_picp* s, int keep_outliers, int n_iters) {
  VO_REQUIRE(s, "null argument");
  VO_REQUIRE(ctx_alive(s->ctx, s->ctx_id), "the context this solver was made on has been destroyed");
  VO_REQUIRE(n_iters >= 0, "negative n_iters");
  if (s->set_n < 0 || !s->shadow_valid)
    return fail(VO_ERR_NOT_READY, "vo_picp_rounds: vo_picp_set_correspondences has not been called");
  if (int r = set_device(s->ctx)) return r;
  if (int r = picp_prepare(s, s->pairs_own.as<int32_t>(), s->set_n, nullptr, keep_outliers, n_iters, true)) return r;
  return picp_enqueue(s, n_iters, true);
}

int vo_picp_graph_info(vo_picp* s, int* use_graph, int* n_graphs, int* n_failures) {
  VO_REQUIRE(s, "null argument");
  if (use_graph) *use_graph = s->use_graph;
  if (n_graphs) *n_graphs = (int)s->graphs.size();
  if (n_failures) *n_failures = s->graph_failures;
  return VO_OK;
}

int voe_picp_submit_info(vo_picp* s, unsigned long long* graph_solves, unsigned long long* plain_solves) {
  VO_REQUIRE(s, "null argument");
  if (graph_solves) *graph_solves = s->graph_solves;
  if (plain_solves) *plain_solves = s->plain_solves;
  return VO_OK;
}

int vo_picp_chain_info(vo_picp* s, int* open_rounds, unsigned long long* speculative, unsigned long long* repeated) {
  VO_REQUIRE(s, "null argument");
  if (open_rounds) *open_rounds = s->chain_len;
  if (speculative) *speculative = s->spec_rounds;
  if (repeated) *repeated = s->spec_redone;
  return VO_OK;
}

int vo_picp_set_exact(vo_picp* s, int on) {
  VO_REQUIRE(s, "null argument");
  VO_REQUIRE(ctx_alive(s->ctx, s->ctx_id), "the context this solver was made on has been destroyed");
  if ((on ? 1 : 0) != s->exact) {          // open rounds belong to the arithmetic they were enqueued in
    if (int r = set_device(s->ctx)) return r;
    if (int r = picp_flush(s)) return r;
  }
  s->exact = on ? 1 : 0;
  return VO_OK;
}

static int picp_read_state(vo_picp* s, PicpState* h) {
  if (int r = picp_flush(s)) return r;
  // one copy up to the end of the tail launch's words (nothing on the host reads the 3 KB of pose history in between: they
  // ride along, cheaper than a second copy)
  VO_HIP_CHECK(hipMemcpyAsync(h, s->d_state, offsetof(PicpState, tail) + sizeof(PicpTail), hipMemcpyDeviceToHost, s->ctx->stream));
  VO_HIP_CHECK(hipStreamSynchronize(s->ctx->stream));
  // a workgroup of the tail launch gave up at its grid barrier (picp.hip, picp_tail_kernel): what the state holds is no result
  if (h->tail.aborted)
    return fail(VO_ERR_HIP, "vo_picp: the tail launch of the last solve gave up waiting at its grid barrier; the results are void "
                            "(VO_PICP_TAIL=0 keeps a launch per round)");
  if (h->n_bad > 0)
    return fail(VO_ERR_BAD_INDEX, "vo_picp: %d correspondence(s) index outside the point arrays", h->n_bad);
  return VO_OK;
}

int vo_picp_get_pose(vo_picp* s, float T[16]) {
  VO_REQUIRE(s && T, "null argument");
  VO_REQUIRE(ctx_alive(s->ctx, s->ctx_id), "the context this solver was made on has been destroyed");
  VO_NOT_CAPTURING(s->ctx);
  if (int r = set_device(s->ctx)) return r;
  PicpState h;
  const int r = picp_read_state(s, &h);
  Pose P;
  for (int i = 0; i < 9; ++i) P.R[i] = h.pose[0][i];
  for (int i = 0; i < 3; ++i) P.t[i] = h.pose[0][9 + i];
  pose_to_T16(P, T);
  return r;
}

int vo_picp_set_pose_dev(vo_picp* s, const float* d_T16) {
  VO_REQUIRE(s && d_T16, "null argument");
  VO_REQUIRE(ctx_alive(s->ctx, s->ctx_id), "the context this solver was made on has been destroyed");
  // consumed by the next solve: folded into its gather launch (or a 12-thread launch of its own)
  if (s->chain_len) { if (int r = set_device(s->ctx)) return r; if (int r = picp_flush(s)) return r; }
  s->pending_T0 = d_T16;
  return VO_OK;
}

int vo_picp_pose_dev_ptr(vo_picp* s, const float** d_T16) {
  VO_REQUIRE(s && d_T16, "null argument");
  VO_REQUIRE(ctx_alive(s->ctx, s->ctx_id), "the context this solver was made on has been destroyed");
  if (s->chain_len) { if (int r = set_device(s->ctx)) return r; if (int r = picp_flush(s)) return r; }
  *d_T16 = s->d_state->T16;
  return VO_OK;
}

__global__ void pose12_to_T16_kernel(const float* p, float* T) {
  const int k = threadIdx.x;
  if (k < 16) {
    const int r = k & 3, c = k >> 2;
    float v;
    if (r == 3) v = (c == 3) ? 1.f : 0.f;
    else if (c == 3) v = p[9 + r];
    else v = p[r + 3 * c];
    T[k] = v;
  }
}

int vo_picp_get_pose_dev(vo_picp* s, float* d_T16) {
  VO_REQUIRE(s && d_T16, "null argument");
  VO_REQUIRE(ctx_alive(s->ctx, s->ctx_id), "the context this solver was made on has been destroyed");
  if (int r = set_device(s->ctx)) return r;
  if (int r = picp_flush(s)) return r;
  hipLaunchKernelGGL(pose12_to_T16_kernel, dim3(1), dim3(64), 0, s->ctx->stream, s->d_state->pose[0], d_T16);
  VO_HIP_CHECK(hipGetLastError());
  return VO_OK;
}

int vo_picp_get_stats(vo_picp* s, float* chi_in, float* chi_out, int* n_in) {
  VO_REQUIRE(s, "null argument");
  VO_REQUIRE(ctx_alive(s->ctx, s->ctx_id), "the context this solver was made on has been destroyed");
  VO_NOT_CAPTURING(s->ctx);
  if (int r = set_device(s->ctx)) return r;
  PicpState h;
  const int r = picp_read_state(s, &h);
  if (chi_in) *chi_in = h.chi_in;
  if (chi_out) *chi_out = h.chi_out;
  if (n_in) *n_in = h.n_in;
  return r;
}

#ifdef VO_STAMPS
// diagnostic build only: copies the s_memtime stamps of the last solve (128 rounds x 8 stamps)
int vo_debug_get_stamps(vo_picp* s, unsigned long long* out) {
  if (int r = picp_flush(s)) return r;
  PicpState h;
  VO_HIP_CHECK(hipMemcpyAsync(&h, s->d_state, sizeof(PicpState), hipMemcpyDeviceToHost, s->ctx->stream));
  VO_HIP_CHECK(hipStreamSynchronize(s->ctx->stream));
  memcpy(out, h.stamps, sizeof(h.stamps));
  return VO_OK;
}
#endif

int vo_picp_get_system(vo_picp* s, float H[36], float b[6]) {
  VO_REQUIRE(s, "null argument");
  VO_REQUIRE(ctx_alive(s->ctx, s->ctx_id), "the context this solver was made on has been destroyed");
  VO_NOT_CAPTURING(s->ctx);
  if (int r = set_device(s->ctx)) return r;
  PicpState h;
  const int r = picp_read_state(s, &h);
  if (H) memcpy(H, h.H, sizeof(h.H));
  if (b) memcpy(b, h.b, sizeof(h.b));
  return r;
}

int vo_picp_batch_set_form(vo_ctx* c, int form) {
  VO_REQUIRE(c, "ctx is null");
  VO_REQUIRE(form >= 0 && form <= 3,
             "form must be 0 (auto), 1 (one launch per round), 2 (one workgroup per problem) or 3 (reference-order arithmetic)");
  c->batch_form = form;
  return VO_OK;
}

int vo_picp_batch_info(vo_ctx* c, int* form, int* workgroups) {
  VO_REQUIRE(c, "ctx is null");
  if (form) *form = c->batch_last_form;
  if (workgroups) *workgroups = c->batch_last_wgs;
  return VO_OK;
}

int vo_picp_batch_help_info(vo_ctx* c, int n_problems, unsigned long long* own, int* n_chunks, int* left_early) {
  VO_REQUIRE(c, "ctx is null");
  VO_NOT_CAPTURING(c);
  VO_REQUIRE(c->batch_last_form == 4 && c->batch_last_help_mode != HELP_SCHED_OFF,
             "the last batched call did not run with helper waves under VO_PICP_HELP_SCHEDULE: it left no record");
  VO_REQUIRE(n_problems == c->batch_last_problems, "n_problems is not the last batched call's");
  if (int r = set_device(c)) return r;
  std::vector<unsigned long long> w((size_t)n_problems * 16);
  VO_HIP_CHECK(hipMemcpyAsync(w.data(), c->batch_help.as<unsigned long long>() + (size_t)c->batch_last_help_rows * 32,
                              sizeof(unsigned long long) * w.size(), hipMemcpyDeviceToHost, c->stream));
  VO_HIP_CHECK(hipStreamSynchronize(c->stream));
  for (int p = 0; p < n_problems; ++p) {
    if (own) own[p] = w[(size_t)p * 16 + 12];
    if (n_chunks) n_chunks[p] = (int)w[(size_t)p * 16 + 13];
    if (left_early) left_early[p] = (int)w[(size_t)p * 16 + 14];
  }
  return VO_OK;
}

static int picp_solve_batch(vo_ctx* c, int n_problems, int rows, int cols, int z_near, int z_far,
                            const float K[9], float thr, int keep_outliers, const float* d_world,
                            size_t world_stride, const float* d_meas, size_t meas_stride,
                            const int32_t* d_pairs, size_t pairs_stride, const int* d_n_pairs,
                            const float* d_T0, int n_iters, float* d_T_out, float* d_stats_out, const float* d_X_world);
// the same in two steps: everything up to (not including) the launches -- workspaces sized, BatchArgs filled, the dropped-
// correspondence counters zeroed on the stream -- so that a caller can hand the arguments to the join as its gather sink
static int picp_batch_prepare(vo_ctx* c, int n_problems, int rows, int cols, int z_near, int z_far,
                              const float K[9], float thr, int keep_outliers, const float* d_world,
                              size_t world_stride, const float* d_meas, size_t meas_stride,
                              const int32_t* d_pairs, size_t pairs_stride, const int* d_n_pairs,
                              const float* d_T0, int n_iters, float* d_T_out, float* d_stats_out, const float* d_X_world,
                              BatchArgs& a);

int vo_picp_solve_batch_dev(vo_ctx* c, int n_problems, int rows, int cols, int z_near, int z_far,
                            const float K[9], float thr, int keep_outliers, const float* d_world,
                            size_t world_stride, const float* d_meas, size_t meas_stride,
                            const int32_t* d_pairs, size_t pairs_stride, const int* d_n_pairs,
                            const float* d_T0, int n_iters, float* d_T_out, float* d_stats_out) {
  return picp_solve_batch(c, n_problems, rows, cols, z_near, z_far, K, thr, keep_outliers, d_world, world_stride, d_meas, meas_stride,
                          d_pairs, pairs_stride, d_n_pairs, d_T0, n_iters, d_T_out, d_stats_out, nullptr);
}

// d_X_world (n_problems x 16, or null): rigid transform applied to every world point the gather fetches
static int picp_solve_batch(vo_ctx* c, int n_problems, int rows, int cols, int z_near, int z_far,
                            const float K[9], float thr, int keep_outliers, const float* d_world,
                            size_t world_stride, const float* d_meas, size_t meas_stride,
                            const int32_t* d_pairs, size_t pairs_stride, const int* d_n_pairs,
                            const float* d_T0, int n_iters, float* d_T_out, float* d_stats_out, const float* d_X_world) {
  BatchArgs a;
  if (int r = picp_batch_prepare(c, n_problems, rows, cols, z_near, z_far, K, thr, keep_outliers, d_world, world_stride, d_meas,
                                 meas_stride, d_pairs, pairs_stride, d_n_pairs, d_T0, n_iters, d_T_out, d_stats_out, d_X_world, a))
    return r;
  if (n_problems == 0) return VO_OK;
  VO_HIP_CHECK(launch_picp_batch(c->stream, a));
  return VO_OK;
}

static int picp_batch_prepare(vo_ctx* c, int n_problems, int rows, int cols, int z_near, int z_far,
                              const float K[9], float thr, int keep_outliers, const float* d_world,
                              size_t world_stride, const float* d_meas, size_t meas_stride,
                              const int32_t* d_pairs, size_t pairs_stride, const int* d_n_pairs,
                              const float* d_T0, int n_iters, float* d_T_out, float* d_stats_out, const float* d_X_world,
                              BatchArgs& a) {
  VO_REQUIRE(c && K, "null argument");
  VO_REQUIRE(n_problems >= 0 && n_iters >= 0, "negative count");
  VO_REQUIRE(n_problems <= 65535, "more than 65535 problems per call (the problem is a grid dimension)");
  if (n_problems == 0) return VO_OK;
  VO_REQUIRE(d_world && d_meas && d_pairs && d_n_pairs && d_T_out, "null device array");
  VO_REQUIRE(world_stride > 0 && meas_stride > 0 && pairs_stride > 0, "zero stride");
  VO_REQUIRE(world_stride < 0x7fffffff && meas_stride < 0x7fffffff && pairs_stride < 0x7fffffff, "stride too large");
  if (int r = set_device(c)) return r;
  a.prepacked = 0;
  a.cam = make_cam(rows, cols, z_near, z_far, K);
  a.thr = thr; a.damping = 1.f; a.keep_outliers = keep_outliers ? 1 : 0;
  a.n_iters = n_iters; a.n_problems = n_problems;
  a.world = d_world; a.world_stride = world_stride;
  a.meas = d_meas; a.meas_stride = meas_stride;
  a.pairs = d_pairs; a.pairs_stride = pairs_stride;
  a.n_pairs = d_n_pairs; a.T0 = d_T0; a.T_out = d_T_out; a.stats_out = d_stats_out;
  a.cap = (pairs_stride + 3) & ~(size_t)3;
  a.n_world = (int)world_stride; a.n_meas = (int)meas_stride;
  VO_HIP_CHECK(c->batch_pack.ensure(sizeof(float) * 5 * a.cap * (size_t)n_problems, c->stream));
  a.packed = c->batch_pack.as<float>();
  a.n_bad = nullptr;
  if (d_stats_out) {
    VO_HIP_CHECK(c->batch_bad.ensure(sizeof(int) * (size_t)n_problems, c->stream));
    VO_HIP_CHECK(hipMemsetAsync(c->batch_bad.p, 0, sizeof(int) * (size_t)n_problems, c->stream));
    a.n_bad = c->batch_bad.as<int>();
  }
  a.states = nullptr; a.partials = nullptr; a.params = nullptr; a.grid = 0; a.exact = 0;
  a.X_world = d_X_world;
  static const int env_form = [] { const char* e = getenv("VO_PICP_BATCH_FORM"); return e ? atoi(e) : 0; }();
  const int form = c->batch_form ? c->batch_form : env_form;
  a.exact = form == 3;
  const bool rounds = form == 1 || (form == 0 && picp_batch_prefers_rounds(n_problems, a.cap, n_iters, c->n_cu));
  if (rounds && !c->capturing) {
    // a few problems: one launch per round with many workgroups per problem (the single-problem kernel with the
    // problem as a grid dimension) instead of one workgroup per problem
    a.grid = picp_grid_for((int)a.cap, c->n_cu);
    const size_t rows = ((size_t)a.grid + 255) & ~(size_t)255;
    const size_t part_bytes = sizeof(float) * PICP_SLOTS * rows * PICP_PSTRIDE * PICP_REPLICAS * (size_t)n_problems;
    const size_t states_cap = c->batch_states.cap;
    VO_HIP_CHECK(c->batch_states.ensure(sizeof(PicpState) * (size_t)n_problems + sizeof(PicpParams), c->stream));
    if (c->batch_states.cap != states_cap) c->batch_params_dev = nullptr;               // reallocated: nothing uploaded yet
    VO_HIP_CHECK(c->batch_partials.ensure(part_bytes, c->stream));
    VO_HIP_CHECK(hipMemsetAsync(c->batch_partials.p, 0, part_bytes, c->stream));       // rows >= grid must read as zero
    PicpParams hp;
    memset(&hp, 0, sizeof(hp));
    hp.cam = a.cam; hp.thr = thr; hp.damping = 1.f; hp.keep_outliers = a.keep_outliers; hp.n_corr = 0;
    PicpParams* d_params = reinterpret_cast<PicpParams*>(c->batch_states.as<char>() + sizeof(PicpState) * (size_t)n_problems);
    if (d_params != c->batch_params_dev || memcmp(&hp, &c->batch_params_host, sizeof(hp)) != 0) {
      // the parameter block changes rarely: upload (and wait, the source is this object) only then
      c->batch_params_host = hp;
      VO_HIP_CHECK(hipMemcpyAsync(d_params, &c->batch_params_host, sizeof(hp), hipMemcpyHostToDevice, c->stream));
      VO_HIP_CHECK(hipStreamSynchronize(c->stream));
      c->batch_params_dev = d_params;
    }
    a.states = c->batch_states.as<PicpState>();
    a.partials = c->batch_partials.as<float>();
    a.params = d_params;
  }
  picp_help_args(a, nullptr, 0);
  if (!a.states && !a.exact && picp_batch_shares(n_problems, a.cap, n_iters, c->n_cu)) {
    // one workgroup per problem would leave CUs without one: their waves take work off the others (picp_batch_shared_kernel)
    VO_HIP_CHECK(c->batch_help.ensure(sizeof(unsigned long long) * picp_help_words(n_problems, c->n_cu), c->stream));
    picp_help_args(a, c->batch_help.as<unsigned long long>(), c->n_cu);
  }
  c->batch_last_form = a.exact ? 3 : a.states ? 1 : a.help_words ? 4 : 2;
  c->batch_last_wgs = a.states ? a.grid * n_problems : a.help_words ? a.help_grid : n_problems;
  c->batch_last_help_rows = a.help_rows; c->batch_last_problems = n_problems; c->batch_last_help_mode = help_sched_mode(a.help_sched);
  return VO_OK;
}

// ---- matcher ------------------------------------------------------------------------------
static int match_workspace(vo_ctx* c, MatchPlan plan, int nt, int nq, int n_frames, void** ws) {
  *ws = nullptr;
  if (plan.search == MatchSearch::Scan) return VO_OK;
  VO_HIP_CHECK(c->prune_ws.ensure(match_workspace_bytes(plan, nt, nq, n_frames), c->stream));
  *ws = c->prune_ws.p;
  return VO_OK;
}

// The one place where the public mode (vo_match_set_mode: 0 auto, 1 full scan, 2 bucket-pruned scan, 3 cell-hash search, 4 / 5
// the exact-duplicate pass first, then 2 / 3) becomes a plan.  nt / nq: the larger / the smaller set (ragged: capacity).
//
// Auto: full scan for small sets; for one frame the bucket-pruned scan (its LDS-tiled scan is the shorter
// dependency chain when the GPU is not full: 82 vs 130 us at 50k x 50k); for many frames per call the cell-hash
// search (25 instead of ~1400 candidates per query: 4.0 vs 4.4 ms per 200 frames, its random accesses hidden
// by occupancy).  In front of either sorted search auto mode runs the exact-duplicate pass (match.hip
// "hash-first": appearances are copied from frame to frame, so almost every query has a bitwise copy in the tree, which
// is its nearest neighbour at distance 0; the search then only sees the queries without one) -- from 8 frames per call on.
// For one frame the pass (three launches, ~45 us at 50k) pays only when NO query is left over: 55 against 78 us; a tracking
// sequence brings new landmarks with every frame, and the sorted search it then still needs costs what it costs without
// the pass (the tree must be sorted for a single open query): 123 against 75 us per frame of the synthetic 200 x 50k
// sequence.  Modes 4 / 5 ask for the pass at any size.
// VO_MATCH_AUTO=2|3 forces one of the sorted searches in auto mode, VO_MATCH_HASH=0 leaves the exact-duplicate pass out,
// VO_MATCH_HASH=1 puts it in front of every sorted search.
//
// Ragged: frames of different sizes: the full scan, or -- from the sizes on where a sorted search pays -- the cell-hash search (its
// workspace is then laid out for the larger capacity in both roles), with the exact-duplicate pass in front of it like
// the rule for equal sizes decides; the bucket-pruned scan takes one size only
static MatchPlan match_plan(const vo_ctx* c, int nt, int nq, int n_frames, bool ragged) {
  MatchSearch search;
  bool pass;
  if (c->match_mode != 0) {
    static const MatchPlan of_mode[6] = {{}, {MatchSearch::Scan, false}, {MatchSearch::Buckets, false}, {MatchSearch::Cells, false},
                                         {MatchSearch::Buckets, true}, {MatchSearch::Cells, true}};
    search = of_mode[c->match_mode].search;
    pass = of_mode[c->match_mode].hash_first;               // 4 / 5: exact-duplicate pass first, at any size it takes
  } else {
    // the full scan: below ~4 M candidate pairs per frame whatever the frame count, and -- a call of one or a few frames, whose
    // sorted searches are a chain of ~8 small launches (45 us) -- up to 1e8 pairs in the whole call: one frame of up to ~10 000 x
    // 10 000 points (measured, one frame, full scan against the sorted searches: 5000: 30 / 46 us, 8500: 36 / 48, 10 000: 42 / 49,
    // 12 000: 60 / 49; tools/match_sizes.py)
    const double pairs = (double)nt * (double)nq;
    // (the 1e8 rule is measured for ONE frame only; calls of 2..7 frames keep the 4 M-pairs-per-frame crossover)
    if (pairs < 4.0e6 || (n_frames <= 1 && pairs < 1.0e8)) return MatchPlan{};
    static const int forced = [] { const char* e = getenv("VO_MATCH_AUTO"); const int v = e ? atoi(e) : 0; return (v == 2 || v == 3) ? v : 0; }();
    search = (forced ? forced == 3 : n_frames >= 8) ? MatchSearch::Cells : MatchSearch::Buckets;
    static const int env = [] { const char* e = getenv("VO_MATCH_HASH"); return e ? (e[0] == '0' ? 0 : 1) : -1; }();
    pass = env < 0 ? n_frames >= 8 : env == 1;
  }
  if (search == MatchSearch::Scan) return MatchPlan{};
  if (ragged) {
    if (!match_cells_supported(nt, nt)) return MatchPlan{};
    search = MatchSearch::Cells;
  } else if (!match_cells_supported(nt, nq)) {              // the cell-hash search serves sets of up to 1.8 M points
    search = MatchSearch::Buckets;
  }
  return MatchPlan{search, pass && match_hash_supported(nt, n_frames)};
}

// the two halves of the steering described at vo_ctx::hint_host, around a batched matcher call in automatic mode
constexpr int HINT_SKIP = 16;
// the plan the call runs: the rule's, or -- while the steering leaves the pass out -- the rule's without the pass
static MatchPlan match_hint_before(vo_ctx* c, MatchPlan plan) {
  static const bool off = [] { const char* e = getenv("VO_MATCH_HINT"); return e && e[0] == '0'; }();
  if (off || c->match_mode != 0 || !plan.hash_first || c->capturing) return plan;
  if (c->hint_pending && hipEventQuery(c->hint_ev) == hipSuccess) {
    c->hint_pending = false;
    if (c->hint_of_skipped_call) {
      if (*c->hint_host != 0) { c->hint_skip_left = 0; c->hint_none_streak = 0; }          // copies are back: the pass again
    } else if (*c->hint_host == 0) {
      if (++c->hint_none_streak >= 2) c->hint_skip_left = HINT_SKIP;                       // twice in a row no frame took the pass: leave it out
    } else {
      c->hint_none_streak = 0;
    }
  }
  (void)hipGetLastError();                        // (hipErrorNotReady of the query is not an error of this call)
  if (c->hint_skip_left > 0) { --c->hint_skip_left; plan.hash_first = false; }      // the plain search: same pairs
  return plan;
}
// plan: what ran; skipped: it ran without the pass because match_hint_before took it out; best / nq_cap / sizes: its keys
static void match_hint_after(vo_ctx* c, MatchPlan plan, bool skipped, const void* ws, int n_frames, const unsigned long long* d_best,
                             size_t best_stride, int nq_cap, const int* d_n1, const int* d_n2) {
  if (c->match_mode != 0 || (!plan.hash_first && !skipped) || c->capturing || !ws || nq_cap <= 0) return;
  if (!c->hint_host) {
    if (hipHostMalloc(reinterpret_cast<void**>(&c->hint_host), 64, hipHostMallocDefault) != hipSuccess ||
        hipMalloc(reinterpret_cast<void**>(&c->hint_dev), 64) != hipSuccess ||
        hipEventCreateWithFlags(&c->hint_ev, hipEventDisableTiming) != hipSuccess) {
      (void)hipGetLastError();
      if (c->hint_host) { (void)hipHostFree(c->hint_host); c->hint_host = nullptr; }      // no steering, nothing else changes
      return;
    }
    *c->hint_host = 1;
  }
  if (c->hint_pending) return;                     // an answer is still on its way
  const hipError_t el = skipped ? launch_match_hint_from_best(c->stream, d_best, best_stride, nq_cap, d_n1, d_n2, n_frames, c->hint_dev)
                                : launch_match_hint(c->stream, ws, n_frames, c->hint_dev);
  c->hint_of_skipped_call = skipped;
  if (el != hipSuccess ||
      hipMemcpyAsync(c->hint_host, c->hint_dev, sizeof(int), hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
      hipEventRecord(c->hint_ev, c->stream) != hipSuccess) { (void)hipGetLastError(); return; }
  c->hint_pending = true;
}

// "Match these frames": the rule's plan, the steering's say on it, the workspace, the launches, the steering's question.
// The caller has sized c->scratch and c->best.  batched: the frames of a many-frames call, cap1 / cap2 rows apart (d_n1 / d_n2:
// their sizes, or null) and steered; otherwise the one frame of vo_match_appearances_dev, which is not.
static int match_frames(vo_ctx* c, bool batched, int n_frames, const float* d_a1, int cap1, const int* d_n1, const float* d_a2,
                        int cap2, const int* d_n2, float radius, int32_t* d_out_pairs, int* d_n_out) {
  const int q = cap1 < cap2 ? cap1 : cap2, nt = cap1 > cap2 ? cap1 : cap2;
  const bool ragged = d_n1 != nullptr;
  const MatchPlan rule = match_plan(c, nt, q, n_frames, ragged);
  const MatchPlan plan = batched ? match_hint_before(c, rule) : rule;
  // (sized for what the rule picks, also while the steering leaves the pass out: the call that brings it back must not have to
  // grow the workspace -- a device allocation of gigabytes and a synchronisation in the middle of a run)
  void* ws = nullptr;
  if (q > 0) if (int r = match_workspace(c, rule, nt, ragged ? nt : q, n_frames, &ws)) return r;
  unsigned long long* best = c->best.as<unsigned long long>();
  if (!batched) {
    VO_HIP_CHECK(launch_match(c->stream, d_a1, cap1, d_a2, cap2, radius, d_out_pairs, d_n_out, best, c->scratch.as<int>(), c->n_cu, ws, plan));
    return VO_OK;
  }
  VO_HIP_CHECK(launch_match_batch(c->stream, d_a1, cap1, 10 * (size_t)cap1, d_a2, cap2, 10 * (size_t)cap2, radius, d_out_pairs,
                                  (size_t)q, d_n_out, best, c->scratch.as<int>(), c->n_cu, ws, n_frames, plan, d_n1, d_n2));
  match_hint_after(c, plan, rule.hash_first && !plan.hash_first, ws, n_frames, best, (size_t)q, q, d_n1, d_n2);
  return VO_OK;
}

int vo_match_set_mode(vo_ctx* c, int mode) {
  VO_REQUIRE(c, "ctx is null");
  VO_REQUIRE(mode >= 0 && mode <= 5, "mode must be 0 (auto), 1 (full scan), 2 (bucket-pruned scan), 3 (cell-hash search), "
                                     "4 / 5 (exact-duplicate pass, then 2 / 3)");
  c->match_mode = mode;
  c->hint_skip_left = 0;              // what the automatic mode learnt from earlier calls is forgotten
  c->hint_none_streak = 0;
  c->hint_pending = false;
  return VO_OK;
}

int vo_match_appearances_dev(vo_ctx* c, const float* d_a1, int n1, const float* d_a2, int n2,
                             float radius, int32_t* d_out_pairs, int* d_n_out) {
  VO_REQUIRE(c && d_n_out, "null argument");
  VO_REQUIRE(n1 >= 0 && n2 >= 0, "negative count");
  VO_REQUIRE((n1 == 0 || d_a1) && (n2 == 0 || d_a2), "null appearance array");
  VO_REQUIRE(aligned8(d_a1, d_a2, d_out_pairs), "device array not on an 8-byte boundary");
  const int nq = n1 < n2 ? n1 : n2;
  VO_REQUIRE(nq == 0 || d_out_pairs, "null output");
  if (int r = set_device(c)) return r;
  if (int r = ensure_scratch(c, nq)) return r;
  VO_HIP_CHECK(c->best.ensure(sizeof(unsigned long long) * (size_t)(nq ? nq : 1), c->stream));
  return match_frames(c, false, 1, d_a1, n1, nullptr, d_a2, n2, nullptr, radius, d_out_pairs, d_n_out);
}

int vo_match_appearances(vo_ctx* c, const float* a1, int n1, const float* a2, int n2, float radius,
                         int32_t* out_pairs, int* n_out) {
  VO_REQUIRE(c && n_out, "null argument");
  VO_NOT_CAPTURING(c);
  VO_REQUIRE(n1 >= 0 && n2 >= 0, "negative count");
  VO_REQUIRE((n1 == 0 || a1) && (n2 == 0 || a2), "null appearance array");
  VO_REQUIRE((n1 == 0 || n2 == 0) || out_pairs, "null output");
  if (int r = set_device(c)) return r;
  const int nq = n1 < n2 ? n1 : n2;
  if (int r = upload(c, c->in[0], a1, sizeof(float) * 10 * (size_t)n1)) return r;
  if (int r = upload(c, c->in[1], a2, sizeof(float) * 10 * (size_t)n2)) return r;
  VO_HIP_CHECK(c->out[0].ensure(sizeof(int32_t) * 2 * (size_t)(nq ? nq : 1), c->stream));
  if (int r = ensure_counts(c)) return r;
  if (int r = vo_match_appearances_dev(c, c->in[0].as<float>(), n1, c->in[1].as<float>(), n2, radius,
                                       c->out[0].as<int32_t>(), c->counts.as<int>()))
    return r;
  int h = 0;
  VO_HIP_CHECK(hipMemcpyAsync(&h, c->counts.p, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  VO_HIP_CHECK(hipStreamSynchronize(c->stream));
  if (h > 0) VO_HIP_CHECK(hipMemcpyAsync(out_pairs, c->out[0].p, sizeof(int32_t) * 2 * (size_t)h, hipMemcpyDeviceToHost, c->stream));
  VO_HIP_CHECK(hipStreamSynchronize(c->stream));
  *n_out = h;
  return VO_OK;
}

// ---- many frame pairs' appearances at once, every pair its own sizes -------------------------
int vo_match_appearances_batch_dev(vo_ctx* c, int n_frames, const float* d_a1, int cap1, const int* d_n1, const float* d_a2,
                                   int cap2, const int* d_n2, float radius, int32_t* d_out_pairs, int* d_n_out) {
  VO_REQUIRE(c && d_n_out, "null argument");
  VO_REQUIRE(n_frames >= 0 && cap1 >= 0 && cap2 >= 0, "negative count");
  if (n_frames == 0) return VO_OK;
  VO_REQUIRE(n_frames <= 65535, "more than 65535 frames per call (the frame is a grid dimension)");
  VO_REQUIRE((d_n1 == nullptr) == (d_n2 == nullptr), "per-frame sizes: give both arrays or neither");
  const int q = cap1 < cap2 ? cap1 : cap2;
  VO_REQUIRE((cap1 == 0 || d_a1) && (cap2 == 0 || d_a2) && (q == 0 || d_out_pairs), "null device array");
  VO_REQUIRE(aligned8(d_a1, d_a2, d_out_pairs), "device array not on an 8-byte boundary");
  if (int r = set_device(c)) return r;
  VO_HIP_CHECK(c->scratch.ensure(sizeof(int) * compaction_scratch_ints(q) * (size_t)n_frames, c->stream));
  VO_HIP_CHECK(c->best.ensure(sizeof(unsigned long long) * (size_t)(q ? q : 1) * (size_t)n_frames, c->stream));
  return match_frames(c, true, n_frames, d_a1, cap1, d_n1, d_a2, cap2, d_n2, radius, d_out_pairs, d_n_out);
}

// ---- batched frames -----------------------------------------------------------------------
static int frames_batch(vo_ctx* c, const vo_frame_batch* b, const vo_frame_sizes* sz);

int vo_frames_batch_dev(vo_ctx* c, const vo_frame_batch* b) { return frames_batch(c, b, nullptr); }

int vo_frames_batch_ragged_dev(vo_ctx* c, const vo_frame_batch* b, const vo_frame_sizes* sizes) {
  VO_REQUIRE(sizes, "null argument");
  VO_REQUIRE(sizes->n_ref && sizes->n_cur && sizes->n_model_pairs, "null per-frame size array");
  return frames_batch(c, b, sizes);
}

}  // extern "C"

static int frames_batch(vo_ctx* c, const vo_frame_batch* b, const vo_frame_sizes* sz) {
  VO_REQUIRE(c && b, "null argument");
  const int F = b->n_frames;
  VO_REQUIRE(F >= 0 && b->n_ref >= 0 && b->n_cur >= 0 && b->n_model >= 0 && b->n_model_pairs >= 0 && b->n_iters >= 0,
             "negative count");
  if (F == 0) return VO_OK;
  VO_REQUIRE(F <= 65535, "more than 65535 frames per call (the frame is a grid dimension)");
  const int q = b->n_ref < b->n_cur ? b->n_ref : b->n_cur;
  VO_REQUIRE(q > 0 && b->n_model > 0, "empty frames");
  VO_REQUIRE(b->ref_app && b->cur_app && b->ref_pts && b->cur_pts && b->model && b->model_pairs, "null input array");
  VO_REQUIRE(b->matches && b->joined && b->poses && b->tri_xyz && b->tri_pairs && b->counts, "null output array");
  VO_REQUIRE(aligned8(b->ref_app, b->cur_app, b->ref_pts, b->cur_pts, b->model_pairs, b->matches, b->joined, b->tri_pairs, b->tri_app),
             "device array not on an 8-byte boundary");
  if (int r = set_device(c)) return r;
  VO_HIP_CHECK(c->scratch.ensure(triangulate_scratch_bytes(q, F), c->stream));    // (covers the counts of the other compactions)
  VO_HIP_CHECK(c->best.ensure(sizeof(unsigned long long) * (size_t)q * (size_t)F, c->stream));
  VO_HIP_CHECK(c->table.ensure(sizeof(unsigned long long) * (size_t)(b->n_ref ? b->n_ref : 1) * (size_t)F, c->stream));
  // ragged frames (sz): the counts of the struct are capacities (= strides), frame f holds sz->n_ref[f] / n_cur[f] points and
  // n_model_pairs[f] model pairs; the matcher (full scan or cell-hash search) picks every frame's roles itself (vo_complete.cpp:15-20)
  int* n_match = b->counts;
  int* n_join = b->counts + F;
  int* n_tri = b->counts + 2 * (size_t)F;
  // compute_correspondences_images, all frames                                  vo_complete.cpp:156
  if (int r = match_frames(c, true, F, b->ref_app, b->n_ref, sz ? sz->n_ref : nullptr, b->cur_app, b->n_cur, sz ? sz->n_cur : nullptr,
                           b->radius, b->matches, n_match))
    return r;
  // X_curr * triangulated_pc                                                    vo_complete.cpp:159
  // The moved cloud as an output is optional: without it the solver's gather applies X_prev to the points it fetches (the
  // same arithmetic, PointCloud.h:80) and the pass that writes n_model points per frame only to re-read the joined ones
  // is gone (117 MB written + 37 us per 200 x 50k frames).
  const float* world = b->model;
  const float* X_world = nullptr;
  if (b->model_moved) {
    VO_HIP_CHECK(launch_transform_batch(c->stream, b->X_prev, b->model, b->n_model, (size_t)b->n_model, b->model_moved, F));
    world = b->model_moved;
  } else {
    X_world = b->X_prev;                              // (null: identity -- the points are used as they are)
  }
  // solver.init(identity) + n rounds: arguments first ...                       vo_complete.cpp:161-164
  BatchArgs pa;
  if (int r = picp_batch_prepare(c, F, b->rows, b->cols, b->z_near, b->z_far, b->K, b->kernel_threshold,
                                 b->keep_outliers, world, (size_t)b->n_model, b->cur_pts, (size_t)b->n_cur,
                                 b->joined, (size_t)q, n_join, nullptr, b->n_iters, b->poses, b->stats, X_world, pa))
    return r;
  // extract_correspondences_world                                               vo_complete.cpp:157
  // ... because the join's writing pass gathers every pair it emits straight into the solver's packed arrays (the one-
  // workgroup-per-problem and reference-order forms; the launch-per-round form of a few frames keeps its own gather pass,
  // which also sets the problems' states up): one launch and one read of the joined pairs less (0.145 + 0.038 -> ~0.15 ms
  // per 200 x 50k frames)
  static const bool fuse_on = [] { const char* e = getenv("VO_JOIN_GATHER"); return !(e && e[0] == '0'); }();
  const bool fuse = fuse_on && pa.states == nullptr && join_fuses_gather(q, b->n_model_pairs, b->n_ref);
  if (fuse) pa.prepacked = 1;
  VO_HIP_CHECK(launch_join_batch(c->stream, b->matches, q, n_match, b->model_pairs, b->n_model_pairs,
                                 sz ? sz->n_model_pairs : nullptr, b->n_ref,
                                 b->joined, n_join, c->table.as<unsigned long long>(), c->scratch.as<int>(), F, (size_t)q,
                                 (size_t)b->n_model_pairs, (size_t)q, fuse ? &pa : nullptr));
  VO_HIP_CHECK(launch_picp_batch(c->stream, pa));
  // triangulate_points with the new pose                                        vo_complete.cpp:172-173
  VO_HIP_CHECK(launch_triangulate_batch(c->stream, b->K, nullptr, b->poses, b->matches, q, n_match, b->ref_pts, b->n_ref,
                                        b->cur_pts, b->n_cur, b->tri_app ? b->cur_app : nullptr, b->tri_xyz, b->tri_pairs,
                                        b->tri_app, n_tri, c->scratch.as<int>(), F, (size_t)q, (size_t)b->n_ref,
                                        (size_t)b->n_cur, (size_t)q));
  return VO_OK;
}

extern "C" {

// ---- join ---------------------------------------------------------------------------------
int vo_join_correspondences_dev(vo_ctx* c, const int32_t* d_img, int n_img, const int* d_n_img,
                                const int32_t* d_world, int n_world, const int* d_n_world, int n_ref,
                                int32_t* d_out, int* d_n_out) {
  VO_REQUIRE(c && d_n_out, "null argument");
  VO_REQUIRE(n_img >= 0 && n_world >= 0 && n_ref >= 0, "negative count");
  VO_REQUIRE((n_img == 0 || (d_img && d_out)) && (n_world == 0 || d_world), "null pair array");
  VO_REQUIRE(aligned8(d_img, d_world, d_out), "device array not on an 8-byte boundary");
  if (int r = set_device(c)) return r;
  VO_HIP_CHECK(c->scratch.ensure(join_scratch_bytes(n_img, 1), c->stream));
  VO_HIP_CHECK(c->table.ensure(sizeof(unsigned long long) * (size_t)(n_ref ? n_ref : 1), c->stream));
  VO_HIP_CHECK(launch_join(c->stream, d_img, n_img, d_n_img, d_world, n_world, d_n_world, n_ref, d_out,
                           d_n_out, c->table.as<unsigned long long>(), c->scratch.as<int>()));
  return VO_OK;
}

int vo_join_correspondences(vo_ctx* c, const int32_t* img, int n_img, const int32_t* world, int n_world,
                            int32_t* out, int* n_out) {
  VO_REQUIRE(c && n_out, "null argument");
  VO_NOT_CAPTURING(c);
  VO_REQUIRE(n_img >= 0 && n_world >= 0, "negative count");
  VO_REQUIRE((n_img == 0 || (img && out)) && (n_world == 0 || world), "null pair array");
  if (int r = set_device(c)) return r;
  // the reference compares arbitrary ints; negative reference indices never match
  // anything meaningful, they are treated as "no partner".
  int n_ref = 0;
  for (int j = 0; j < n_world; ++j) if (world[2 * j] >= n_ref) n_ref = world[2 * j] + 1;
  if (int r = upload(c, c->in[0], img, sizeof(int32_t) * 2 * (size_t)n_img)) return r;
  if (int r = upload(c, c->in[1], world, sizeof(int32_t) * 2 * (size_t)n_world)) return r;
  VO_HIP_CHECK(c->out[0].ensure(sizeof(int32_t) * 2 * (size_t)(n_img ? n_img : 1), c->stream));
  if (int r = ensure_counts(c)) return r;
  if (int r = vo_join_correspondences_dev(c, c->in[0].as<int32_t>(), n_img, nullptr, c->in[1].as<int32_t>(),
                                          n_world, nullptr, n_ref, c->out[0].as<int32_t>(), c->counts.as<int>()))
    return r;
  int h = 0;
  VO_HIP_CHECK(hipMemcpyAsync(&h, c->counts.p, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  VO_HIP_CHECK(hipStreamSynchronize(c->stream));
  if (h > 0) VO_HIP_CHECK(hipMemcpyAsync(out, c->out[0].p, sizeof(int32_t) * 2 * (size_t)h, hipMemcpyDeviceToHost, c->stream));
  VO_HIP_CHECK(hipStreamSynchronize(c->stream));
  *n_out = h;
  return VO_OK;
}

// ---- radius search (fullSearch) ----------------------------------------------------------------
int vo_radius_search_dev(vo_ctx* c, const float* d_tree, int n_tree, const float* d_qry, int n_q, float radius,
                         int32_t* d_offsets, int32_t* d_indices, int capacity) {
  VO_REQUIRE(c && d_offsets, "null argument");
  VO_REQUIRE(n_tree >= 0 && n_q >= 0 && capacity >= 0, "negative count");
  VO_REQUIRE((n_tree == 0 || d_tree) && (n_q == 0 || d_qry) && (capacity == 0 || d_indices), "null array");
  VO_REQUIRE(match_cells_supported(n_tree, n_q), "more than 1 835 008 points in one set");
  VO_REQUIRE(aligned8(d_tree, d_qry), "device array not on an 8-byte boundary");       // (the cell-hash path loads rows as 8-byte words)
  if (int r = set_device(c)) return r;
  void* ws = nullptr;
  if (n_tree > 0 && n_q > 0) if (int r = match_workspace(c, MatchPlan{MatchSearch::Cells, false}, n_tree, n_q, 1, &ws)) return r;
  VO_HIP_CHECK(launch_radius_search(c->stream, d_tree, n_tree, d_qry, n_q, radius, d_offsets, d_indices, capacity, ws));
  return VO_OK;
}

int vo_radius_search(vo_ctx* c, const float* tree, int n_tree, const float* qry, int n_q, float radius,
                     int32_t* offsets, int32_t* indices, int capacity, int* n_total) {
  VO_REQUIRE(c && offsets && n_total, "null argument");
  VO_NOT_CAPTURING(c);
  VO_REQUIRE(n_tree >= 0 && n_q >= 0 && capacity >= 0, "negative count");
  VO_REQUIRE((n_tree == 0 || tree) && (n_q == 0 || qry) && (capacity == 0 || indices), "null array");
  if (int r = set_device(c)) return r;
  if (int r = upload(c, c->in[0], tree, sizeof(float) * 10 * (size_t)n_tree)) return r;
  if (int r = upload(c, c->in[1], qry, sizeof(float) * 10 * (size_t)n_q)) return r;
  VO_HIP_CHECK(c->out[0].ensure(sizeof(int32_t) * ((size_t)n_q + 1), c->stream));
  VO_HIP_CHECK(c->out[1].ensure(sizeof(int32_t) * (size_t)(capacity ? capacity : 1), c->stream));
  if (int r = vo_radius_search_dev(c, c->in[0].as<float>(), n_tree, c->in[1].as<float>(), n_q, radius,
                                   c->out[0].as<int32_t>(), c->out[1].as<int32_t>(), capacity))
    return r;
  VO_HIP_CHECK(hipMemcpyAsync(offsets, c->out[0].p, sizeof(int32_t) * ((size_t)n_q + 1), hipMemcpyDeviceToHost, c->stream));
  VO_HIP_CHECK(hipStreamSynchronize(c->stream));
  *n_total = offsets[n_q];
  if (*n_total > capacity)
    return fail(VO_ERR_INVALID_ARG, "vo_radius_search: %d hits, room for %d", *n_total, capacity);
  if (*n_total > 0)
    VO_HIP_CHECK(hipMemcpyAsync(indices, c->out[1].p, sizeof(int32_t) * (size_t)*n_total, hipMemcpyDeviceToHost, c->stream));
  VO_HIP_CHECK(hipStreamSynchronize(c->stream));
  return VO_OK;
}

// ---- transform ------------------------------------------------------------------------------
int vo_transform_points_dev(vo_ctx* c, const float T[16], const float* d_T16, const float* d_in, int n,
                            const int* d_n, float* d_out) {
  VO_REQUIRE(c && (T || d_T16), "null argument");
  VO_REQUIRE(n >= 0 && (n == 0 || (d_in && d_out)), "bad point arrays");
  if (int r = set_device(c)) return r;
  if (d_T16) VO_HIP_CHECK(launch_transform_points_devpose(c->stream, d_T16, d_in, n, d_n, d_out));
  else VO_HIP_CHECK(launch_transform_points(c->stream, pose_from_T16(T), d_in, n, d_n, d_out));
  return VO_OK;
}

int vo_transform_points(vo_ctx* c, const float T[16], const float* in, int n, float* out) {
  VO_REQUIRE(c && T, "null argument");
  VO_NOT_CAPTURING(c);
  VO_REQUIRE(n >= 0 && (n == 0 || (in && out)), "bad point arrays");
  if (n == 0) return VO_OK;
  if (int r = set_device(c)) return r;
  if (int r = upload(c, c->in[0], in, sizeof(float) * 3 * (size_t)n)) return r;
  VO_HIP_CHECK(c->out[0].ensure(sizeof(float) * 3 * (size_t)n, c->stream));
  if (int r = vo_transform_points_dev(c, T, nullptr, c->in[0].as<float>(), n, nullptr, c->out[0].as<float>())) return r;
  VO_HIP_CHECK(hipMemcpyAsync(out, c->out[0].p, sizeof(float) * 3 * (size_t)n, hipMemcpyDeviceToHost, c->stream));
  VO_HIP_CHECK(hipStreamSynchronize(c->stream));
  return VO_OK;
}

// ---- triangulation ----------------------------------------------------------------------------
int vo_triangulate_dev(vo_ctx* c, const float K[9], const float X[16], const float* d_X16,
                       const int32_t* d_pairs, int n, const int* d_n, const float* d_p1, int n1,
                       const float* d_p2, int n2, const float* d_app2, float* d_out_xyz,
                       int32_t* d_out_pairs, float* d_out_app, int* d_n_out) {
  VO_REQUIRE(c && K && d_n_out, "null argument");
  VO_REQUIRE(X || d_X16, "no pose given");
  VO_REQUIRE(n >= 0 && n1 >= 0 && n2 >= 0, "negative count");
  VO_REQUIRE(n == 0 || (d_pairs && d_p1 && d_p2 && d_out_xyz), "null device array");
  VO_REQUIRE(aligned8(d_pairs, d_p1, d_p2, d_app2, d_out_app) && aligned8(d_out_pairs), "device array not on an 8-byte boundary");
  if (int r = set_device(c)) return r;
  VO_HIP_CHECK(c->scratch.ensure(triangulate_scratch_bytes(n, 1), c->stream));
  Pose Xp;
  if (X) Xp = pose_from_T16(X);
  VO_HIP_CHECK(launch_triangulate(c->stream, K, X ? &Xp : nullptr, d_X16, d_pairs, n, d_n, d_p1, n1, d_p2,
                                  n2, d_app2, d_out_xyz, d_out_pairs, d_out_app, d_n_out,
                                  c->scratch.as<int>()));
  return VO_OK;
}

int vo_triangulate(vo_ctx* c, const float K[9], const float X[16], const int32_t* pairs, int n,
                   const float* p1, int n1, const float* p2, int n2, const float* app2, float* out_xyz,
                   int32_t* out_pairs, float* out_app, int* n_out) {
  VO_REQUIRE(c && K && X && n_out, "null argument");
  VO_NOT_CAPTURING(c);
  VO_REQUIRE(n >= 0 && n1 >= 0 && n2 >= 0, "negative count");
  VO_REQUIRE(n == 0 || (pairs && p1 && p2 && out_xyz), "null array");
  if (int r = set_device(c)) return r;
  const bool want_app = app2 && out_app;
  if (int r = upload(c, c->in[0], pairs, sizeof(int32_t) * 2 * (size_t)n)) return r;
  if (int r = upload(c, c->in[1], p1, sizeof(float) * 2 * (size_t)n1)) return r;
  if (int r = upload(c, c->in[2], p2, sizeof(float) * 2 * (size_t)n2)) return r;
  if (want_app) if (int r = upload(c, c->in[3], app2, sizeof(float) * 10 * (size_t)n2)) return r;
  const size_t nn = (size_t)(n ? n : 1);
  VO_HIP_CHECK(c->out[0].ensure(sizeof(float) * 3 * nn, c->stream));
  VO_HIP_CHECK(c->out[1].ensure(sizeof(int32_t) * 2 * nn, c->stream));
  if (want_app) VO_HIP_CHECK(c->out[2].ensure(sizeof(float) * 10 * nn, c->stream));
  if (int r = ensure_counts(c)) return r;
  if (int r = vo_triangulate_dev(c, K, X, nullptr, c->in[0].as<int32_t>(), n, nullptr, c->in[1].as<float>(),
                                 n1, c->in[2].as<float>(), n2, want_app ? c->in[3].as<float>() : nullptr,
                                 c->out[0].as<float>(), out_pairs ? c->out[1].as<int32_t>() : nullptr,
                                 want_app ? c->out[2].as<float>() : nullptr, c->counts.as<int>()))
    return r;
  int h = 0;
  VO_HIP_CHECK(hipMemcpyAsync(&h, c->counts.p, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  VO_HIP_CHECK(hipStreamSynchronize(c->stream));
  if (h > 0) {
    VO_HIP_CHECK(hipMemcpyAsync(out_xyz, c->out[0].p, sizeof(float) * 3 * (size_t)h, hipMemcpyDeviceToHost, c->stream));
    if (out_pairs) VO_HIP_CHECK(hipMemcpyAsync(out_pairs, c->out[1].p, sizeof(int32_t) * 2 * (size_t)h, hipMemcpyDeviceToHost, c->stream));
    if (want_app) VO_HIP_CHECK(hipMemcpyAsync(out_app, c->out[2].p, sizeof(float) * 10 * (size_t)h, hipMemcpyDeviceToHost, c->stream));
    VO_HIP_CHECK(hipStreamSynchronize(c->stream));
  }
  *n_out = h;
  return VO_OK;
}

// ---- epipolar initialisation (epipolar_utils.cpp:176-213) --------------------------------------
// Device half first (epi.hip): maxima of both images, the 45 sums of A^T A, one small read-back; then the host's 9 x 9
// eigen-solve, rank-2 projection and decomposition of E in double (include/vo/epipolar.hpp); then ONE launch that counts,
// for all four candidates at once, the correspondences that triangulate in front of both cameras; a second read-back.
int vo_estimate_transform_dev(vo_ctx* c, const float K[9], const int32_t* d_pairs, int n_max, const int* d_n, const float* d_p1,
                              int n1, const float* d_p2, int n2, float X_out[16]) {
  VO_REQUIRE(c && K && d_pairs && d_p1 && d_p2 && X_out, "null argument");
  VO_NOT_CAPTURING(c);
  VO_REQUIRE(n_max >= 8, "fewer than 8 correspondences");
  VO_REQUIRE(n1 > 0 && n2 > 0, "empty point set");
  VO_REQUIRE(aligned8(d_pairs, d_p1, d_p2), "device arrays must be 8-byte aligned");
  if (int r = set_device(c)) return r;
  VO_HIP_CHECK(c->epi_ws.ensure(epi_workspace_bytes(), c->stream));
  VO_HIP_CHECK(launch_epi_front(c->stream, d_pairs, n_max, d_n, d_p1, n1, d_p2, n2, c->epi_ws.p));
  struct { unsigned maxima[4]; int info[4]; int votes[8]; double ata[45]; } h;
  static_assert(sizeof(h) == 64 + 45 * sizeof(double), "layout of the epipolar workspace");
  VO_HIP_CHECK(hipMemcpyAsync(&h, c->epi_ws.p, sizeof(h), hipMemcpyDeviceToHost, c->stream));
  VO_HIP_CHECK(hipStreamSynchronize(c->stream));
  if (h.info[1] > 0)
    return fail(VO_ERR_BAD_INDEX, "vo_estimate_transform: %d pair(s) index outside the point arrays", h.info[1]);
  if (h.info[0] < 8) return fail(VO_ERR_INVALID_ARG, "vo_estimate_transform: fewer than 8 correspondences (%d)", h.info[0]);
  std::vector<double> AtA(81, 0.0);
  for (int i = 0, k = 0; i < 9; ++i)
    for (int j = i; j < 9; ++j, ++k) AtA[(size_t)i * 9 + j] = AtA[(size_t)j * 9 + i] = h.ata[k];
  float mx[4];
  memcpy(mx, h.maxima, sizeof(mx));
  vo::Matrix3f k;
  for (int j = 0; j < 9; ++j) k.m[j] = K[j];
  const vo::Matrix3f F = vo::fundamental_from_normal_matrix(AtA, vo::conditioning_matrix(mx[0], mx[1]), vo::conditioning_matrix(mx[2], mx[3]));
  vo::Isometry3f X[4];
  vo::transform_candidates(k, F, X);
  Pose P[4];
  for (int q = 0; q < 4; ++q) P[q] = pose_from_T16(X[q].data());
  VO_HIP_CHECK(launch_epi_vote(c->stream, K, P, d_pairs, n_max, d_n, d_p1, n1, d_p2, n2, c->epi_ws.p));
  int votes[4] = {0, 0, 0, 0};
  VO_HIP_CHECK(hipMemcpyAsync(votes, static_cast<char*>(c->epi_ws.p) + 32, sizeof(votes), hipMemcpyDeviceToHost, c->stream));
  VO_HIP_CHECK(hipStreamSynchronize(c->stream));
  const vo::Isometry3f best = vo::pick_candidate(X, votes);
  memcpy(X_out, best.data(), sizeof(float) * 16);
  return VO_OK;
}

// the host forms refuse a pair outside its point arrays before anything is uploaded: first index against n_a, second against n_b
static int check_pair_range(const char* fn, const int32_t* pairs, int n, int n_a, int n_b) {
  for (int i = 0; i < n; ++i)
    if (pairs[2 * i] < 0 || pairs[2 * i] >= n_a || pairs[2 * i + 1] < 0 || pairs[2 * i + 1] >= n_b)
      return fail(VO_ERR_BAD_INDEX, "%s: pair %d = (%d,%d) outside the point arrays", fn, i, pairs[2 * i], pairs[2 * i + 1]);
  return VO_OK;
}

int vo_estimate_transform(vo_ctx* c, const float K[9], const int32_t* pairs, int n, const float* p1, int n1,
                          const float* p2, int n2, float X_out[16]) {
  VO_REQUIRE(c && K && pairs && p1 && p2 && X_out, "null argument");
  VO_NOT_CAPTURING(c);
  VO_REQUIRE(n >= 8, "fewer than 8 correspondences");
  VO_REQUIRE(n1 > 0 && n2 > 0, "empty point set");
  if (int r = check_pair_range("vo_estimate_transform", pairs, n, n1, n2)) return r;
  if (int r = set_device(c)) return r;
  if (int r = upload(c, c->in[0], pairs, sizeof(int32_t) * 2 * (size_t)n)) return r;
  if (int r = upload(c, c->in[1], p1, sizeof(float) * 2 * (size_t)n1)) return r;
  if (int r = upload(c, c->in[2], p2, sizeof(float) * 2 * (size_t)n2)) return r;
  return vo_estimate_transform_dev(c, K, c->in[0].as<int32_t>(), n, nullptr, c->in[1].as<float>(), n1, c->in[2].as<float>(), n2, X_out);
}

// ---- RANSAC in front of the epipolar initialisation (ransac.hip) ---------------------------------------------------------
// gather -> hypotheses -> scoring -> selection -> mask and compaction: one read-back (live pairs, bad indices, winner, inliers);
// then vo_estimate_transform_dev itself on the compacted inlier pairs, which makes the result that of vo_estimate_transform
// on those pairs bit for bit.
int ransac_check_params(const vo_ransac_params* p) {
  if (p->n_hypotheses < 1 || p->n_hypotheses > 65536)
    return fail(VO_ERR_INVALID_ARG, "vo_estimate_transform_ransac: n_hypotheses %d outside 1 .. 65536", p->n_hypotheses);
  if (!(p->threshold_px > 0.f) || !std::isfinite(p->threshold_px))
    return fail(VO_ERR_INVALID_ARG, "vo_estimate_transform_ransac: threshold_px must be positive and finite (%g)", (double)p->threshold_px);
  return VO_OK;
}

int vo_estimate_transform_ransac_dev(vo_ctx* c, const float K[9], const int32_t* d_pairs, int n_max, const int* d_n,
                                     const float* d_p1, int n1, const float* d_p2, int n2, const vo_ransac_params* params,
                                     float X_out[16], uint8_t* d_mask, int32_t* d_counts, int* n_inliers) {
  VO_REQUIRE(c && K && d_pairs && d_p1 && d_p2 && params && X_out, "null argument");
  VO_NOT_CAPTURING(c);
  VO_REQUIRE(n_max >= 8, "fewer than 8 correspondences");
  VO_REQUIRE(n1 > 0 && n2 > 0, "empty point set");
  VO_REQUIRE(aligned8(d_pairs, d_p1, d_p2), "device arrays must be 8-byte aligned");
  if (int r = ransac_check_params(params)) return r;
  if (int r = set_device(c)) return r;
  const int H = params->n_hypotheses;
  VO_HIP_CHECK(c->ransac_ws.ensure(ransac_workspace_bytes(n_max, H), c->stream));
  RansacArgs a = ransac_layout(c->ransac_ws.p, n_max, H);
  a.pairs = d_pairs; a.d_n = d_n; a.p1 = d_p1; a.n1 = n1; a.p2 = d_p2; a.n2 = n2;
  a.seed = params->seed; a.thr2 = params->threshold_px * params->threshold_px;
  if (d_mask) a.mask = d_mask;
  if (d_counts) a.counts = d_counts;
  VO_HIP_CHECK(launch_ransac(c->stream, a));
  int info[8];
  VO_HIP_CHECK(hipMemcpyAsync(info, a.info, sizeof(info), hipMemcpyDeviceToHost, c->stream));
  VO_HIP_CHECK(hipStreamSynchronize(c->stream));
  if (info[1] > 0)
    return fail(VO_ERR_BAD_INDEX, "vo_estimate_transform_ransac: %d pair(s) index outside the point arrays", info[1]);
  if (info[0] < 8) return fail(VO_ERR_INVALID_ARG, "vo_estimate_transform_ransac: fewer than 8 correspondences (%d)", info[0]);
  if (info[2] < 0) return fail(VO_ERR_INVALID_ARG, "vo_estimate_transform_ransac: no valid hypothesis among %d", H);
  if (info[4] < 8)
    return fail(VO_ERR_INVALID_ARG, "vo_estimate_transform_ransac: the best hypothesis (%d) has %d inlier(s), fewer than 8", info[2], info[4]);
  if (int r = vo_estimate_transform_dev(c, K, a.out_pairs, info[4], nullptr, d_p1, n1, d_p2, n2, X_out)) return r;
  if (n_inliers) *n_inliers = info[4];
  return VO_OK;
}

int vo_estimate_transform_ransac(vo_ctx* c, const float K[9], const int32_t* pairs, int n, const float* p1, int n1,
                                 const float* p2, int n2, const vo_ransac_params* params, float X_out[16], uint8_t* inlier_mask,
                                 int* n_inliers) {
  VO_REQUIRE(c && K && pairs && p1 && p2 && params && X_out, "null argument");
  VO_NOT_CAPTURING(c);
  VO_REQUIRE(n >= 8, "fewer than 8 correspondences");
  VO_REQUIRE(n1 > 0 && n2 > 0, "empty point set");
  if (int r = ransac_check_params(params)) return r;
  if (int r = check_pair_range("vo_estimate_transform_ransac", pairs, n, n1, n2)) return r;
  if (int r = set_device(c)) return r;
  if (int r = upload(c, c->in[0], pairs, sizeof(int32_t) * 2 * (size_t)n)) return r;
  if (int r = upload(c, c->in[1], p1, sizeof(float) * 2 * (size_t)n1)) return r;
  if (int r = upload(c, c->in[2], p2, sizeof(float) * 2 * (size_t)n2)) return r;
  if (inlier_mask) VO_HIP_CHECK(c->out[0].ensure((size_t)n, c->stream));
  if (int r = vo_estimate_transform_ransac_dev(c, K, c->in[0].as<int32_t>(), n, nullptr, c->in[1].as<float>(), n1, c->in[2].as<float>(),
                                               n2, params, X_out, inlier_mask ? c->out[0].as<uint8_t>() : nullptr, nullptr, n_inliers))
    return r;
  if (inlier_mask) {
    VO_HIP_CHECK(hipMemcpyAsync(inlier_mask, c->out[0].p, (size_t)n, hipMemcpyDeviceToHost, c->stream));
    VO_HIP_CHECK(hipStreamSynchronize(c->stream));
  }
  return VO_OK;
}

// ---- P3P RANSAC in front of the tracking solve (pose_ransac.hip) ---------------------------------------------------------------
// gather -> hypotheses -> scoring -> selection (status, pose handed on) -> mask and compaction, all on the stream: the device
// form never reads back, so it falls back to the plain frame (identity pose, every live pair) where the host form refuses.
static int pose_ransac_camera(int rows, int cols, int z_near, int z_far, const float K[9], CamK& cam, double Kinv[9]) {
  for (int i = 0; i < 9; ++i) cam.K[i] = K[i];
  cam.rows = rows; cam.cols = cols; cam.z_near = z_near; cam.z_far = z_far;
  if (!invert_k(K, Kinv)) return fail(VO_ERR_INVALID_ARG, "vo_estimate_pose_ransac: K is singular");
  return VO_OK;
}

// the caller's side of a PoseRansacArgs that a layout function has carved: camera, inputs, parameters and outputs
static void pose_ransac_fill(PoseRansacArgs& a, const CamK& cam, const double Kinv[9], const float* d_world, int n_world,
                             const float* d_meas, int n_meas, const int32_t* d_pairs, const int* d_n, const vo_ransac_params* params,
                             float* d_T16, int32_t* d_inl, int* d_n_inl, uint8_t* d_mask, int32_t* d_counts, int* d_status) {
  a.cam = cam;
  for (int i = 0; i < 9; ++i) a.Kinv[i] = Kinv[i];
  a.pairs = d_pairs; a.d_n = d_n; a.world = d_world; a.n_world = n_world; a.meas = d_meas; a.n_meas = n_meas;
  a.seed = params->seed; a.thr2 = params->threshold_px * params->threshold_px;
  a.out_pairs = d_inl; a.n_out = d_n_inl; a.T_out = d_T16; a.status = d_status;
  if (d_mask) a.mask = d_mask;
  if (d_counts) a.counts = d_counts;
}

int vo_estimate_pose_ransac_dev(vo_ctx* c, int rows, int cols, int z_near, int z_far, const float K[9], const float* d_world,
                                int n_world, const float* d_meas, int n_meas, const int32_t* d_pairs, int n_max, const int* d_n,
                                const vo_ransac_params* params, float* d_T16, int32_t* d_inl, int* d_n_inl, uint8_t* d_mask,
                                int32_t* d_counts, int* d_status) {
  VO_REQUIRE(c && K && d_world && d_meas && d_pairs && params && d_T16 && d_inl && d_n_inl && d_status, "null argument");
  VO_REQUIRE(n_max >= 1, "n_max must be positive");
  VO_REQUIRE(n_world >= 0 && n_meas >= 0, "negative point count");
  VO_REQUIRE(aligned8(d_pairs, d_meas, d_inl), "device arrays must be 8-byte aligned");
  if (int r = ransac_check_params(params)) return r;
  const int H = params->n_hypotheses;
  CamK cam;
  double Kinv[9];
  if (int r = pose_ransac_camera(rows, cols, z_near, z_far, K, cam, Kinv)) return r;
  const size_t need = pose_ransac_workspace_bytes(n_max, H);
  if (c->capturing && c->pose_ws.cap < need)
    return fail(VO_ERR_NOT_READY, "vo_estimate_pose_ransac_dev: the workspace would have to grow inside a graph capture (make one "
                                  "call with n_max %d and %d hypotheses before capturing)", n_max, H);
  if (int r = set_device(c)) return r;
  VO_HIP_CHECK(c->pose_ws.ensure(need, c->stream));
  PoseRansacArgs a = pose_ransac_layout(c->pose_ws.p, n_max, H);
  pose_ransac_fill(a, cam, Kinv, d_world, n_world, d_meas, n_meas, d_pairs, d_n, params, d_T16, d_inl, d_n_inl, d_mask, d_counts,
                   d_status);
  VO_HIP_CHECK(launch_pose_ransac(c->stream, a));
  return VO_OK;
}

int vo_estimate_pose_ransac(vo_ctx* c, int rows, int cols, int z_near, int z_far, const float K[9], const float* world, int n_world,
                            const float* meas, int n_meas, const int32_t* pairs, int n, const vo_ransac_params* params,
                            float T_out[16], uint8_t* inlier_mask, int* n_inliers) {
  VO_REQUIRE(c && K && params && T_out, "null argument");
  VO_NOT_CAPTURING(c);
  if (n < 4) return fail(VO_ERR_INVALID_ARG, "vo_estimate_pose_ransac: fewer than 4 correspondences (%d)", n);
  VO_REQUIRE(pairs && world && meas, "null argument");
  VO_REQUIRE(n_world > 0 && n_meas > 0, "empty point set");
  if (int r = ransac_check_params(params)) return r;
  if (int r = check_pair_range("vo_estimate_pose_ransac", pairs, n, n_meas, n_world)) return r;
  if (int r = set_device(c)) return r;
  if (int r = upload(c, c->in[0], pairs, sizeof(int32_t) * 2 * (size_t)n)) return r;
  if (int r = upload(c, c->in[1], world, sizeof(float) * 3 * (size_t)n_world)) return r;
  if (int r = upload(c, c->in[2], meas, sizeof(float) * 2 * (size_t)n_meas)) return r;
  VO_HIP_CHECK(c->out[0].ensure((size_t)n, c->stream));
  VO_HIP_CHECK(c->out[1].ensure(sizeof(int32_t) * 2 * (size_t)n, c->stream));
  VO_HIP_CHECK(c->out[2].ensure(128, c->stream));
  float* d_res = c->out[2].as<float>();                    // [0, 16) pose, [16] inlier count, [17] status
  int* d_res_i = c->out[2].as<int>();
  if (int r = vo_estimate_pose_ransac_dev(c, rows, cols, z_near, z_far, K, c->in[1].as<float>(), n_world, c->in[2].as<float>(), n_meas,
                                          c->in[0].as<int32_t>(), n, nullptr, params, d_res, c->out[1].as<int32_t>(), d_res_i + 16,
                                          c->out[0].as<uint8_t>(), nullptr, d_res_i + 17))
    return r;
  float res[18];
  VO_HIP_CHECK(hipMemcpyAsync(res, d_res, sizeof(res), hipMemcpyDeviceToHost, c->stream));
  VO_HIP_CHECK(hipStreamSynchronize(c->stream));
  int cnt, st;
  std::memcpy(&cnt, &res[16], sizeof(int));
  std::memcpy(&st, &res[17], sizeof(int));
  if (st == VO_POSE_RANSAC_BAD_INDEX) return fail(VO_ERR_BAD_INDEX, "vo_estimate_pose_ransac: a pair indexes outside the point arrays");
  if (st == VO_POSE_RANSAC_FEW_PAIRS) return fail(VO_ERR_INVALID_ARG, "vo_estimate_pose_ransac: fewer than 4 correspondences");
  if (st == VO_POSE_RANSAC_NO_HYPOTHESIS)
    return fail(VO_ERR_INVALID_ARG, "vo_estimate_pose_ransac: no valid hypothesis among %d", params->n_hypotheses);
  if (st == VO_POSE_RANSAC_FEW_INLIERS)
    return fail(VO_ERR_INVALID_ARG, "vo_estimate_pose_ransac: the best hypothesis has %d inlier(s), fewer than 6", cnt);
  if (st != VO_POSE_RANSAC_OK) return fail(VO_ERR_HIP, "vo_estimate_pose_ransac: unexpected status %d", st);
  std::memcpy(T_out, res, sizeof(float) * 16);
  if (inlier_mask) {
    VO_HIP_CHECK(hipMemcpyAsync(inlier_mask, c->out[0].p, (size_t)n, hipMemcpyDeviceToHost, c->stream));
    VO_HIP_CHECK(hipStreamSynchronize(c->stream));
  }
  if (n_inliers) *n_inliers = cnt;
  return VO_OK;
}

// ---- Gauss-Newton refit of the relative pose on the Sampson error (epi_refine.hip) -----------------------------------------------
// 2 (n_rounds + 1) launches on the stream and nothing else: the start pose travels in the launch arguments or is read from
// device memory, the state and the workgroup rows live in the context's workspace, pose and statistics are written by the
// last launch.
static int refine_check_params(const vo_epi_refine_params* p) {
  if (p->n_rounds < 1 || p->n_rounds > 100)
    return fail(VO_ERR_INVALID_ARG, "vo_refine_transform: n_rounds %d outside 1 .. 100", p->n_rounds);
  if (!(p->huber_px >= 0.f) || !std::isfinite(p->huber_px))
    return fail(VO_ERR_INVALID_ARG, "vo_refine_transform: huber_px must be >= 0 and finite (%g)", (double)p->huber_px);
  return VO_OK;
}

int vo_refine_transform_dev(vo_ctx* c, const float K[9], const int32_t* d_pairs, int n_max, const int* d_n, const uint8_t* d_mask,
                            const float* d_p1, int n1, const float* d_p2, int n2, const float X_in[16], const float* d_X_in,
                            const vo_epi_refine_params* params, float* d_X_out, vo_epi_refine_stats* d_stats) {
  VO_REQUIRE(c && K && d_pairs && d_p1 && d_p2 && params && d_X_out && d_stats, "null argument");
  VO_REQUIRE((X_in != nullptr) != (d_X_in != nullptr), "exactly one of X_in and d_X_in must be given");
  VO_REQUIRE(n_max >= 1, "n_max must be positive");
  VO_REQUIRE(n1 >= 0 && n2 >= 0, "negative point count");
  VO_REQUIRE(aligned8(d_pairs, d_p1, d_p2, d_stats), "device arrays must be 8-byte aligned");
  if (int r = refine_check_params(params)) return r;
  RefineArgs a{};
  {
    double Kinv[9];
    if (!invert_k(K, Kinv)) return fail(VO_ERR_INVALID_ARG, "vo_refine_transform: K is singular");
    for (int r = 0; r < 3; ++r)
      for (int q = 0; q < 3; ++q) a.Kinv[3 * r + q] = Kinv[r + 3 * q];
  }
  const size_t need = epi_refine_workspace_bytes(n_max);
  if (c->capturing && c->refine_ws.cap < need)
    return fail(VO_ERR_NOT_READY, "vo_refine_transform_dev: the workspace would have to grow inside a graph capture (make one "
                                  "call with n_max %d before capturing)", n_max);
  if (int r = set_device(c)) return r;
  VO_HIP_CHECK(c->refine_ws.ensure(need, c->stream));
  a.pairs = d_pairs; a.n_max = n_max; a.d_n = d_n; a.mask = d_mask; a.p1 = d_p1; a.n1 = n1; a.p2 = d_p2; a.n2 = n2;
  if (X_in) memcpy(a.X_in, X_in, sizeof(a.X_in));
  a.d_X_in = d_X_in;
  a.n_rounds = params->n_rounds; a.huber = (double)params->huber_px;
  a.X_out = d_X_out; a.stats = d_stats;
  VO_HIP_CHECK(launch_epi_refine(c->stream, a, c->refine_ws.p));
  return VO_OK;
}

int vo_refine_transform(vo_ctx* c, const float K[9], const int32_t* pairs, int n, const uint8_t* mask, const float* p1, int n1,
                        const float* p2, int n2, const float X_in[16], const vo_epi_refine_params* params, float X_out[16],
                        vo_epi_refine_stats* stats_out) {
  VO_REQUIRE(c && K && pairs && p1 && p2 && X_in && params && X_out && stats_out, "null argument");
  VO_NOT_CAPTURING(c);
  VO_REQUIRE(n >= 1, "n must be positive");
  VO_REQUIRE(n1 > 0 && n2 > 0, "empty point set");
  if (int r = refine_check_params(params)) return r;
  if (int r = set_device(c)) return r;
  if (int r = upload(c, c->in[0], pairs, sizeof(int32_t) * 2 * (size_t)n)) return r;
  if (int r = upload(c, c->in[1], p1, sizeof(float) * 2 * (size_t)n1)) return r;
  if (int r = upload(c, c->in[2], p2, sizeof(float) * 2 * (size_t)n2)) return r;
  if (mask)
    if (int r = upload(c, c->in[3], mask, (size_t)n)) return r;
  VO_HIP_CHECK(c->out[2].ensure(128, c->stream));
  struct { float X[16]; vo_epi_refine_stats s; } h;
  static_assert(sizeof(h) == 104, "pose and statistics come back in one copy");
  char* d_res = c->out[2].as<char>();
  if (int r = vo_refine_transform_dev(c, K, c->in[0].as<int32_t>(), n, nullptr, mask ? c->in[3].as<uint8_t>() : nullptr,
                                      c->in[1].as<float>(), n1, c->in[2].as<float>(), n2, X_in, nullptr, params,
                                      reinterpret_cast<float*>(d_res), reinterpret_cast<vo_epi_refine_stats*>(d_res + 64)))
    return r;
  VO_HIP_CHECK(hipMemcpyAsync(&h, d_res, sizeof(h), hipMemcpyDeviceToHost, c->stream));
  VO_HIP_CHECK(hipStreamSynchronize(c->stream));
  memcpy(X_out, h.X, sizeof(h.X));
  *stats_out = h.s;
  return VO_OK;
}

// The batched form: P problems in one fixed set of launches (pose_ransac.hip), every problem held to the single call above
// bit for bit.  The argument checks come first and touch neither the context nor the device.
static int pose_ransac_batch_check(const void* c, int n_problems, const float* K, const float* d_world, size_t world_stride, int n_world,
                                   const float* d_meas, size_t meas_stride, int n_meas, const int32_t* d_pairs, size_t pairs_stride,
                                   const vo_ransac_params* params, const float* d_T16, const int32_t* d_inl, const int* d_n_inl,
                                   const int* d_status) {
  const char* fn = "vo_estimate_pose_ransac_batch_dev";
  if (!(c && K && d_world && d_meas && d_pairs && params && d_T16 && d_inl && d_n_inl && d_status))
    return fail(VO_ERR_INVALID_ARG, "%s: null argument", fn);
  if (n_problems < 1) return fail(VO_ERR_INVALID_ARG, "%s: n_problems must be positive (%d)", fn, n_problems);
  if (n_problems > 65535) return fail(VO_ERR_INVALID_ARG, "%s: more than 65535 problems per call (the problem is a grid dimension)", fn);
  if (n_world < 0 || n_meas < 0) return fail(VO_ERR_INVALID_ARG, "%s: negative point count", fn);
  if (pairs_stride < 1) return fail(VO_ERR_INVALID_ARG, "%s: pairs_stride must be positive", fn);
  if (world_stride >= 0x7fffffff || meas_stride >= 0x7fffffff || pairs_stride >= 0x7fffffff)
    return fail(VO_ERR_INVALID_ARG, "%s: stride too large", fn);
  if (world_stride < (size_t)n_world || meas_stride < (size_t)n_meas)
    return fail(VO_ERR_INVALID_ARG, "%s: a stride is smaller than its point count (world %zu < %d or meas %zu < %d)", fn, world_stride,
                n_world, meas_stride, n_meas);
  if (!aligned8(d_pairs, d_meas, d_inl)) return fail(VO_ERR_INVALID_ARG, "%s: device arrays must be 8-byte aligned", fn);
  return ransac_check_params(params);
}

static int pose_ransac_batch(vo_ctx* c, int n_problems, int rows, int cols, int z_near, int z_far, const float K[9], const float* d_world,
                             size_t world_stride, int n_world, const float* d_meas, size_t meas_stride, int n_meas,
                             const int32_t* d_pairs, size_t pairs_stride, const int* d_n, const vo_ransac_params* params, float* d_T16,
                             int32_t* d_inl, int* d_n_inl, uint8_t* d_mask, int32_t* d_counts, int* d_status) {
  if (int r = pose_ransac_batch_check(c, n_problems, K, d_world, world_stride, n_world, d_meas, meas_stride, n_meas, d_pairs, pairs_stride,
                                      params, d_T16, d_inl, d_n_inl, d_status))
    return r;
  const int H = params->n_hypotheses, n_max = (int)pairs_stride;
  CamK cam;
  double Kinv[9];
  if (int r = pose_ransac_camera(rows, cols, z_near, z_far, K, cam, Kinv)) return r;
  const size_t need = pose_ransac_batch_workspace_bytes(n_problems, n_max, H);
  if (c->capturing && c->pose_batch_ws.cap < need)
    return fail(VO_ERR_NOT_READY, "vo_estimate_pose_ransac_batch_dev: the workspace would have to grow inside a graph capture (make "
                                  "one call with %d problems of stride %d and %d hypotheses before capturing)", n_problems, n_max, H);
  if (int r = set_device(c)) return r;
  VO_HIP_CHECK(c->pose_batch_ws.ensure(need, c->stream));
  PoseRansacBatchArgs b = pose_ransac_batch_layout(c->pose_batch_ws.p, n_problems, n_max, H);
  pose_ransac_fill(b.a, cam, Kinv, d_world, n_world, d_meas, n_meas, d_pairs, d_n, params, d_T16, d_inl, d_n_inl, d_mask, d_counts,
                   d_status);
  b.world_stride = world_stride; b.meas_stride = meas_stride; b.pairs_stride = pairs_stride;
  VO_HIP_CHECK(launch_pose_ransac_batch(c->stream, b));
  return VO_OK;
}

int vo_estimate_pose_ransac_batch_dev(vo_ctx* c, int n_problems, int rows, int cols, int z_near, int z_far, const float K[9],
                                      const float* d_world, size_t world_stride, int n_world, const float* d_meas, size_t meas_stride,
                                      int n_meas, const int32_t* d_pairs, size_t pairs_stride, const int* d_n,
                                      const vo_ransac_params* params, float* d_T16, int32_t* d_inl, int* d_n_inl, uint8_t* d_mask,
                                      int32_t* d_counts, int* d_status) {
  return pose_ransac_batch(c, n_problems, rows, cols, z_near, z_far, K, d_world, world_stride, n_world, d_meas, meas_stride, n_meas,
                           d_pairs, pairs_stride, d_n, params, d_T16, d_inl, d_n_inl, d_mask, d_counts, d_status);
}

// ---- the many-frames call with robust tracking: the stages of frames_batch with the batched RANSAC between the join and the
// solve.  The join is the plain one (the pairs are filtered before the solver packs them) and the moved cloud is always
// written, because the RANSAC gather reads it.
int vo_frames_batch_track_dev(vo_ctx* c, const vo_frame_batch* b, const vo_frame_sizes* sz, const vo_frame_track* t) {
  VO_REQUIRE(c && b && t, "null argument");
  VO_REQUIRE(t->status && t->n_tracked, "null tracking output array");
  VO_REQUIRE(!sz || (sz->n_ref && sz->n_cur && sz->n_model_pairs), "null per-frame size array");
  const int F = b->n_frames;
  VO_REQUIRE(F >= 0 && b->n_ref >= 0 && b->n_cur >= 0 && b->n_model >= 0 && b->n_model_pairs >= 0 && b->n_iters >= 0,
             "negative count");
  if (int r = ransac_check_params(&t->ransac)) return r;
  if (F == 0) return VO_OK;
  VO_REQUIRE(F <= 65535, "more than 65535 frames per call (the frame is a grid dimension)");
  const int q = b->n_ref < b->n_cur ? b->n_ref : b->n_cur;
  VO_REQUIRE(q > 0 && b->n_model > 0, "empty frames");
  VO_REQUIRE(b->ref_app && b->cur_app && b->ref_pts && b->cur_pts && b->model && b->model_pairs, "null input array");
  VO_REQUIRE(b->matches && b->joined && b->poses && b->tri_xyz && b->tri_pairs && b->counts, "null output array");
  VO_REQUIRE(aligned8(b->ref_app, b->cur_app, b->ref_pts, b->cur_pts, b->model_pairs, b->matches, b->joined, b->tri_pairs, b->tri_app,
                      t->tracked_pairs),
             "device array not on an 8-byte boundary");
  if (int r = set_device(c)) return r;
  // what the caller did not ask for lives in the context: moved cloud | tracked pairs | winners (256-aligned blocks)
  const size_t moved_bytes = b->model_moved ? 0 : up256(sizeof(float) * 3 * (size_t)b->n_model * (size_t)F);
  const size_t pairs_bytes = t->tracked_pairs ? 0 : up256(sizeof(int32_t) * 2 * (size_t)q * (size_t)F);
  const size_t win_bytes = t->T_winner ? 0 : sizeof(float) * 16 * (size_t)F;
  const size_t track_need = moved_bytes + pairs_bytes + win_bytes;
  if (c->capturing && c->track_ws.cap < track_need)
    return fail(VO_ERR_NOT_READY, "vo_frames_batch_track_dev: the workspace would have to grow inside a graph capture (make one call "
                                  "with the same sizes before capturing)");
  VO_HIP_CHECK(c->track_ws.ensure(track_need, c->stream));
  float* moved = b->model_moved ? b->model_moved : c->track_ws.as<float>();
  int32_t* tracked = t->tracked_pairs ? t->tracked_pairs : reinterpret_cast<int32_t*>(c->track_ws.as<char>() + moved_bytes);
  float* winners = t->T_winner ? t->T_winner : reinterpret_cast<float*>(c->track_ws.as<char>() + moved_bytes + pairs_bytes);
  VO_HIP_CHECK(c->scratch.ensure(triangulate_scratch_bytes(q, F), c->stream));
  VO_HIP_CHECK(c->best.ensure(sizeof(unsigned long long) * (size_t)q * (size_t)F, c->stream));
  VO_HIP_CHECK(c->table.ensure(sizeof(unsigned long long) * (size_t)(b->n_ref ? b->n_ref : 1) * (size_t)F, c->stream));
  int* n_match = b->counts;
  int* n_join = b->counts + F;
  int* n_tri = b->counts + 2 * (size_t)F;
  // 1. match and join, as frames_batch
  if (int r = match_frames(c, true, F, b->ref_app, b->n_ref, sz ? sz->n_ref : nullptr, b->cur_app, b->n_cur, sz ? sz->n_cur : nullptr,
                           b->radius, b->matches, n_match))
    return r;
  VO_HIP_CHECK(launch_join_batch(c->stream, b->matches, q, n_match, b->model_pairs, b->n_model_pairs,
                                 sz ? sz->n_model_pairs : nullptr, b->n_ref,
                                 b->joined, n_join, c->table.as<unsigned long long>(), c->scratch.as<int>(), F, (size_t)q,
                                 (size_t)b->n_model_pairs, (size_t)q, nullptr));
  // 2. X_prev * model, always materialised
  VO_HIP_CHECK(launch_transform_batch(c->stream, b->X_prev, b->model, b->n_model, (size_t)b->n_model, moved, F));
  // 3. the batched RANSAC on (moved cloud, cur_pts, joined, counts[1])
  if (int r = pose_ransac_batch(c, F, b->rows, b->cols, b->z_near, b->z_far, b->K, moved, (size_t)b->n_model, b->n_model, b->cur_pts,
                                (size_t)b->n_cur, b->n_cur, b->joined, (size_t)q, n_join, &t->ransac, winners, tracked, t->n_tracked,
                                nullptr, nullptr, t->status))
    return r;
  // 4. the batched solve from the winners on the pairs handed on
  if (int r = picp_solve_batch(c, F, b->rows, b->cols, b->z_near, b->z_far, b->K, b->kernel_threshold, b->keep_outliers, moved,
                               (size_t)b->n_model, b->cur_pts, (size_t)b->n_cur, tracked, (size_t)q, t->n_tracked, winners, b->n_iters,
                               b->poses, b->stats, nullptr))
    return r;
  // 5. triangulation with the final pose
  VO_HIP_CHECK(launch_triangulate_batch(c->stream, b->K, nullptr, b->poses, b->matches, q, n_match, b->ref_pts, b->n_ref,
                                        b->cur_pts, b->n_cur, b->tri_app ? b->cur_app : nullptr, b->tri_xyz, b->tri_pairs,
                                        b->tri_app, n_tri, c->scratch.as<int>(), F, (size_t)q, (size_t)b->n_ref,
                                        (size_t)b->n_cur, (size_t)q));
  return VO_OK;
}

}  // extern "C"
